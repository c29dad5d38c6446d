// fixedlag.hip -- fixed-lag smoothing: the joint Gaussian factor on one state
// (gtsam::LinearContainerFactor over the keys x_i, v_i: gpslam_hip_add_state_gaussians), the marginalisation of the chain's head into
// such a factor on the oldest kept state (gtsam::BatchFixedLagSmoother's elimination of the old variables at the current
// linearisation: gpslam_hip_marginalize_head), and the growth of the chain at its tail (gpslam_hip_append_states).  On a handle with
// landmarks the same pair exists over the keys (x_i, v_i, l_0 .. l_{L-1}): gpslam_hip_add_border_gaussians, and the head's
// marginalisation onto the oldest kept state and the landmarks (gpslam_hip_marginalize_head_onto_landmarks, k_head_schur_border).
// fp64 handles only, one unsharded handle off the segmented landmark path; a translation unit of its own, so that every other
// kernel of the library keeps its bytes.  No atomics, every sum in a fixed order: two calls give bit-identical results.
#include "api_common.hpp"

#include <cfloat>
#include <numeric>

namespace impl64 {
#include "api_decl.inc"
}

namespace {

// ------------------------------------------------------------------ the factor
// r = A xi - c,  xi = [Local(pose_lin, pose_i) ; vel_i - vel_lin];  rows [A | 0] on left state i.  One thread per factor.
struct SgArgs {
  const double *pose, *vel;
  int stride, count, chart;
  const int *idx, *row0;
  const double *lin;      // count x (pd + d): [pose_lin | vel_lin]
  const double *A, *c;    // count x b x b, count x b
  double *rowLR, *rowE;   // the full-width row table (JAC)
  double *partial;        // per-block error partial sums
};
template <int MF, bool JAC> __global__ void __launch_bounds__(128) k_state_gauss(SgArgs a) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, b = 2 * d;
  const int f = blockIdx.x * 128 + threadIdx.x;
  double err = 0.0;
  if (f < a.count) {
    const int i = a.idx[f];
    const double *lin = a.lin + (size_t)f * (pd + d);
    double x[pd], xl[pd], xi[b], Hd[1];
#pragma unroll
    for (int k = 0; k < pd; k++) { x[k] = a.pose[(size_t)k * a.stride + i]; xl[k] = lin[k]; }
    PoseFactors<double, MF, false>::prior(xl, x, a.chart, xi, Hd);     // Local(pose_lin, pose_i) in the handle's chart
#pragma unroll
    for (int k = 0; k < d; k++) xi[d + k] = a.vel[(size_t)k * a.stride + i] - lin[pd + k];
    const double *Af = a.A + (size_t)f * b * b, *cf = a.c + (size_t)f * b;
    const int row0 = JAC ? a.row0[f] : 0;
    for (int r = 0; r < b; r++) {
      double res = -cf[r];
#pragma unroll
      for (int q = 0; q < b; q++) res += Af[r * b + q] * xi[q];
      err += res * res;
      if (JAC) {
        a.rowE[row0 + r] = res;
        double *row = a.rowLR + (size_t)(row0 + r) * 2 * b;
#pragma unroll
        for (int q = 0; q < b; q++) { row[q] = Af[r * b + q]; row[b + q] = 0.0; }
      }
    }
  }
  const double tot = block_sum(0.5 * err);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = tot;
}

// ------------------------------------------------------------------ the factor over one state and the landmarks
// r = A xi - c,  xi = [Local(pose_lin, pose_i) ; vel_i - vel_lin ; l - lm_lin],  n = b + nl <= kBgMaxN.  One workgroup of one wave, the
// factors one after the other (a handle carries one or two): lane 0 forms the pose part of xi, the lanes d .. n - 1 the differences,
// then lane t row t of the residual.  The Jacobian pass's residuals stay on the device for k_border_inject / k_border_schur / k_head_sums.
constexpr int kBgMaxN = 12 + kMaxRhs - 1;
struct BgArgs {
  const double *pose, *vel, *lmk;
  int stride, count, chart, nl;
  const int *idx;
  const double *lin;      // count x (pd + d + nl): [pose_lin | vel_lin | lm_lin]
  const double *A, *c;    // count x n x n, count x n
  double *r;              // count x n
  double *partial;        // one error partial sum
};
// JAC: the Jacobian pass, whose residuals are the linearisation's and are kept; an error-only pass (a Levenberg-Marquardt trial point)
// must leave them as they are -- a rejected trial re-assembles from them
template <int MF, bool JAC> __global__ void __launch_bounds__(64) k_border_gauss(BgArgs a) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, b = 2 * d;
  __shared__ double xi[kBgMaxN];
  const int t = threadIdx.x, n = b + a.nl;
  double err = 0.0;
  for (int f = 0; f < a.count; f++) {
    const int i = a.idx[f];
    const double *lin = a.lin + (size_t)f * (pd + d + a.nl);
    if (t == 0) {
      double x[pd], xl[pd], xp[b], Hd[1];
#pragma unroll
      for (int k = 0; k < pd; k++) { x[k] = a.pose[(size_t)k * a.stride + i]; xl[k] = lin[k]; }
      PoseFactors<double, MF, false>::prior(xl, x, a.chart, xp, Hd);     // Local(pose_lin, pose_i) in the handle's chart
#pragma unroll
      for (int k = 0; k < d; k++) xi[k] = xp[k];
    } else if (t >= d && t < b) {
      xi[t] = a.vel[(size_t)(t - d) * a.stride + i] - lin[pd + t - d];
    } else if (t >= b && t < n) {
      xi[t] = a.lmk[t - b] - lin[pd + d + t - b];
    }
    __syncthreads();
    if (t < n) {
      const double *row = a.A + ((size_t)f * n + t) * n;
      double res = -a.c[(size_t)f * n + t];
      for (int q = 0; q < n; q++) res += row[q] * xi[q];
      if (JAC) a.r[(size_t)f * n + t] = res;
      err += res * res;
    }
    __syncthreads();
  }
  const double tot = block_sum(0.5 * err);
  if (t == 0) a.partial[0] = tot;
}

// Behind the assembly: record idx += [A_x^T A_x | . | -A_x^T r | A_x^T A_L] (columns 0 .. nl of the right-hand sides; the closure
// columns behind them stay).  One workgroup; a thread owns the same entries for every factor, which it takes in order.
struct BgPatchArgs {
  int count, nl, B, R;
  const int *idx;
  const double *A, *r;
  double *blk, *gsave;    // the level-0 records; the gradient copy or null
  const double *x;        // level-0 solutions (k_border_schur)
  double *S, *gL;         // [S (nl x R) | gL (nl)] (k_border_schur)
};
__global__ void __launch_bounds__(256) k_border_inject(BgPatchArgs a) {
  const int B = a.B, BB = B * B, n = B + a.nl, ne = BB + B * (1 + a.nl);
  const size_t BS = (size_t)2 * BB + (size_t)B * a.R;
  for (int e = threadIdx.x; e < ne; e += 256) {
    const bool isD = e < BB;
    const int col = isD ? e % B : (e - BB) / B, k = isD ? e / B : (e - BB) % B;     // D[k][col]; G column col, row k
    for (int f = 0; f < a.count; f++) {
      const double *A = a.A + (size_t)f * n * n, *r = a.r + (size_t)f * n;
      const int i = a.idx[f];
      double *rec = a.blk + (size_t)i * BS;
      double acc = 0.0;
      if (isD) {
        for (int m = 0; m < n; m++) acc += A[m * n + k] * A[m * n + col];
        rec[e] += acc;
      } else if (col == 0) {
        for (int m = 0; m < n; m++) acc -= A[m * n + k] * r[m];
        rec[2 * BB + k] += acc;
        if (a.gsave) a.gsave[(size_t)i * B + k] += acc;
      } else {
        for (int m = 0; m < n; m++) acc += A[m * n + k] * A[m * n + B + col - 1];
        rec[2 * BB + col * B + k] += acc;
      }
    }
  }
}
// Behind k_lm_reduce: S[al][c] += sum over the factor's rows of A_L[row, al] (v - A_x[row, :] X_i[:, c]), v = -r[row] (c = 0), A_L[row, c - 1]
// (1 <= c <= nl), 0 (a closure column); gL[al] += -A_L^T r.  One thread per (al, c), the factors and their rows in order.
__global__ void __launch_bounds__(256) k_border_schur(BgPatchArgs a) {
  const int tid = blockIdx.x * 256 + threadIdx.x;
  if (tid >= a.nl * a.R) return;
  const int al = tid / a.R, c = tid - al * a.R, B = a.B, n = B + a.nl;
  double acc = 0.0, g = 0.0;
  for (int f = 0; f < a.count; f++) {
    const double *A = a.A + (size_t)f * n * n, *r = a.r + (size_t)f * n;
    const double *X = a.x + ((size_t)a.idx[f] * a.R + c) * B;
    for (int m = 0; m < n; m++) {
      const double aL = A[m * n + B + al];
      double u = 0.0;
      for (int k = 0; k < B; k++) u += A[m * n + k] * X[k];
      const double v = c == 0 ? -r[m] : (c <= a.nl ? A[m * n + B + c - 1] : 0.0);
      acc += aL * (v - u);
      if (c == 0) g -= aL * r[m];
    }
  }
  a.S[(size_t)al * a.R + c] += acc;
  if (c == 0) a.gL[al] += g;
}

// ------------------------------------------------------------------ the head's share of block k
// out = [D_k^left (B x B) | g_k^left (B)]: R^T R and -R^T e over the right halves of the rows whose left state is k - 1, the
// full-width table first, then the compact one (pose columns only), each in table order
template <int B> __global__ void __launch_bounds__(64) k_head_left(const int *rowptr, const double *rowLR, const double *rowE, const int *crowptr,
                                                                    const double *rowC, const double *rowCE, int k, double *out) {
  constexpr int BB = B * B, Dh = B / 2, NE = (BB + B + 63) / 64;
  const int r0 = rowptr[k - 1], r1 = rowptr[k], c0 = crowptr[k - 1], c1 = crowptr[k];
#pragma unroll
  for (int t = 0; t < NE; t++) {
    const int e = threadIdx.x + 64 * t;
    if (e >= BB + B) continue;
    const bool isg = e >= BB;
    const int r = isg ? e - BB : e / B, c = isg ? 0 : e % B;
    double acc = 0.0;
    for (int rho = r0; rho < r1; rho++) {
      const double *row = rowLR + (size_t)rho * 2 * B + B;
      acc += isg ? -row[r] * rowE[rho] : row[r] * row[c];
    }
    if (r < Dh && (isg || c < Dh))
      for (int rho = c0; rho < c1; rho++) {
        const double *row = rowC + (size_t)rho * B + Dh;
        acc += isg ? -row[r] * rowCE[rho] : row[r] * row[c];
      }
    out[e] = acc;
  }
}

// ------------------------------------------------------------------ the Schur recursion
// One wave.  State: S = D'_i, s = g'_i.  Step i < k: the augmented matrix M = [S | O_i^T | s] (B x (2B + 1)) goes through a
// row-oriented Cholesky elimination -- pivot row j scaled by 1 / sqrt(pivot), then taken out of the rows below -- which leaves
// [L^T | V | w], V = L^-1 O_i^T, w = L^-1 s; then D'_{i+1} = D_{i+1} - V^T V, g'_{i+1} = g_{i+1} - V^T w.  O_i = H_{i+1,i} as the
// records store it.  Block k's raw values are the head's share (k_head_left), not the record's.  The raw blocks of step i + 1
// are requested into registers before the arithmetic of step i and reach LDS behind it.
// out = [Lambda (B x B) | g'_k (B)]; a non-positive pivot raises *flag.
template <int B> __global__ void __launch_bounds__(64) k_head_schur(const double *blk, int BS, int k, const double *left, double *out, int *flag) {
  constexpr int BB = B * B, W = 2 * B + 1, NM = (B * W + 63) / 64, NB = (BB + 63) / 64;
  __shared__ double M[B * W], Dn[BB], gn[B];
  const int t = threadIdx.x;
  double rO[NB], rD[NB], rg;
  auto fetch = [&](int i) {     // O_i, D_{i+1}, g_{i+1}; clamped, unconditional loads
    const double *p = blk + (size_t)i * BS;
    const bool last = i + 1 == k;
    const double *pn = last ? left : blk + (size_t)(i + 1) * BS;
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const int e = min(t + 64 * u, BB - 1);
      rO[u] = p[BB + e];
      rD[u] = pn[e];
    }
    rg = pn[(last ? BB : 2 * BB) + min(t, B - 1)];
  };
  for (int e = t; e < BB; e += 64) M[(e / B) * W + e % B] = blk[e];
  if (t < B) M[t * W + 2 * B] = blk[2 * BB + t];
  fetch(0);
  for (int i = 0; i < k; i++) {
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const int e = t + 64 * u;
      if (e < BB) { M[(e % B) * W + B + e / B] = rO[u]; Dn[e] = rD[u]; }    // O_i^T
    }
    if (t < B) gn[t] = rg;
    __syncthreads();
    if (i + 1 < k) fetch(i + 1);
    for (int j = 0; j < B; j++) {
      double piv = M[j * W + j];
      if (!(piv > 0.0)) { if (t == 0) *flag = 1; piv = 1.0; }
      const double pinv = 1.0 / piv, sinv = 1.0 / sqrt(piv);
      double v[NM];
#pragma unroll
      for (int u = 0; u < NM; u++) {
        const int e = t + 64 * u;
        if (e < B * W) {
          const int r = e / W, c = e - r * W;
          const double m = M[e];
          if (r < j || c < j) v[u] = m;
          else if (r == j) v[u] = m * sinv;
          else v[u] = m - M[j * W + r] * M[j * W + c] * pinv;
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < NM; u++) {
        const int e = t + 64 * u;
        if (e < B * W) M[e] = v[u];
      }
      __syncthreads();
    }
    double nS[NB], ns = 0.0;
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const int e = t + 64 * u;
      if (e < BB) {
        const int r = e / B, c = e % B;
        double acc = Dn[e];
        for (int q = 0; q < B; q++) acc -= M[q * W + B + r] * M[q * W + B + c];
        nS[u] = acc;
      }
    }
    if (t < B) {
      ns = gn[t];
      for (int q = 0; q < B; q++) ns -= M[q * W + B + t] * M[q * W + 2 * B];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const int e = t + 64 * u;
      if (e < BB) M[(e / B) * W + e % B] = nS[u];
    }
    if (t < B) M[t * W + 2 * B] = ns;
    __syncthreads();
  }
  for (int e = t; e < BB; e += 64) out[e] = M[(e / B) * W + e % B];
  if (t < B) out[BB + t] = M[t * W + 2 * B];
}

// ------------------------------------------------------------------ the head onto the landmarks
// left[B^2 + B (1 + q) + r] = B_k^left[r][q]: the rows whose left state is k - 1 and that name a landmark, right half (transposed) times
// rowM -- the layout of a record's right-hand-side columns, behind k_head_left's [D_k^left | g_k^left]
__global__ void __launch_bounds__(256) k_head_left_lm(const int *rowptr, const double *rowLR, const double *rowM, const int *rowLm, int B, int ld, int nl, int k,
                                                       double *left) {
  const int r0 = rowptr[k - 1], r1 = rowptr[k];
  for (int e = threadIdx.x; e < B * nl; e += 256) {
    const int q = e / B, r = e - q * B, lm = q / ld, qq = q - lm * ld;
    double acc = 0.0;
    for (int rho = r0; rho < r1; rho++)
      if (rowLm[rho] == lm) acc += rowLR[(size_t)rho * 2 * B + B + r] * rowM[(size_t)rho * ld + qq];
    left[B * B + B * (1 + q) + r] = acc;
  }
}
// out = [H_LL^head (nl x nl) | g_L^head (nl)]: rowM^T rowM and -rowM^T rowE over the full-width rows of the states < k that name a
// landmark, in table order, then the landmark blocks A_L^T A_L, -A_L^T r of the border Gaussians with idx < k, in their order.
// One thread per entry.
__global__ void __launch_bounds__(256) k_head_sums(const int *rowptr, const double *rowM, const double *rowE, const int *rowLm, int ld, int nl, int k, int B,
                                                    int count, const int *idx, const double *A, const double *r, double *out) {
  const int tid = blockIdx.x * 256 + threadIdx.x;
  if (tid >= nl * (nl + 1)) return;
  const int al = tid / (nl + 1), c = tid - al * (nl + 1);      // c = 0: the gradient
  const int lm = al / ld, q = al - lm * ld, cl = c - 1, n = B + nl;
  const bool same = c >= 1 && cl / ld == lm;
  const int q2 = same ? cl - lm * ld : 0;
  double acc = 0.0;
  if (c == 0 || same) {
    const int r1 = rowptr[k];
    for (int rho = rowptr[0]; rho < r1; rho++) {
      if (rowLm[rho] != lm) continue;
      const double m = rowM[(size_t)rho * ld + q];
      acc += c == 0 ? -m * rowE[rho] : m * rowM[(size_t)rho * ld + q2];
    }
  }
  for (int f = 0; f < count; f++) {
    if (idx[f] >= k) continue;
    const double *Af = A + (size_t)f * n * n, *rf = r + (size_t)f * n;
    for (int m = 0; m < n; m++) acc += c == 0 ? -Af[m * n + B + al] * rf[m] : Af[m * n + B + al] * Af[m * n + B + cl];
  }
  out[c == 0 ? nl * nl + al : al * nl + cl] = acc;
}

// (B = 6, 12.)  The recursion of k_head_schur with the landmark columns carried along: G_i = [g_i | B_i] (B x (1 + nl), a record's right-hand-side
// columns 0 .. nl; the closure columns behind them are not read).  Four waves.  Step i < k: the augmented matrix
// M = [S | O_i^T | G] (B x (2B + 1 + nl), at most 12 x 52, row stride W) goes through the row-oriented Cholesky elimination, which leaves
// [L^T | V | Wg]; then S <- D_{i+1} - V^T V, G <- G_{i+1} - V^T Wg and T += Wg^T Wg, T ((1 + nl) x (1 + nl)) in registers, entry
// t + 256 u with thread t, summed in the order of i (both halves: the two copies of an entry see the same products in the same order).
// nl is a runtime value: every index is checked against the live extent, lanes beyond it neither read nor write.  Block k's raw
// values are the head's share (left: k_head_left, k_head_left_lm).  The raw blocks of step i + 1 are requested before step i's arithmetic.
// out = [Lambda (n x n, n = B + nl) | g' (n)], Lambda = [[S, G[:, 1:]], [., H_LL^head - T[1:, 1:]]], g' = [G[:, 0] ; g_L^head - T[1:, 0]]
// (head = [H_LL^head | g_L^head], k_head_sums); a non-positive pivot raises *flag.
template <int B> __global__ void __launch_bounds__(256) k_head_schur_border(const double *blk, int BS, int k, int nl, const double *left, const double *head,
                                                                            double *out, int *flag) {
  constexpr int NT = 256, BB = B * B, WM = 2 * B + kMaxRhs;
  constexpr int NM = (B * WM + NT - 1) / NT, NB = (BB + NT - 1) / NT, NG = (B * kMaxRhs + NT - 1) / NT, NTT = (kMaxRhs * kMaxRhs + NT - 1) / NT;
  __shared__ double M[B * WM], Dn[BB], Gn[B * kMaxRhs];
  const int t = threadIdx.x, R1 = 1 + nl, W = 2 * B + R1, n = B + nl;
  double rO[NB], rD[NB], rG[NG], T[NTT];
#pragma unroll
  for (int u = 0; u < NTT; u++) T[u] = 0.0;
#pragma unroll
  for (int u = 0; u < NG; u++) rG[u] = 0.0;
  auto fetch = [&](int i) {     // O_i, D_{i+1}, G_{i+1}
    const double *p = blk + (size_t)i * BS;
    const bool last = i + 1 == k;
    const double *pn = last ? left : blk + (size_t)(i + 1) * BS;
    const double *pg = pn + (last ? BB : 2 * BB);
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const int e = min(t + NT * u, BB - 1);
      rO[u] = p[BB + e];
      rD[u] = pn[e];
    }
#pragma unroll
    for (int u = 0; u < NG; u++) {
      const int e = t + NT * u;
      if (e < B * R1) rG[u] = pg[e];
    }
  };
  for (int e = t; e < BB; e += NT) M[(e / B) * W + e % B] = blk[e];
  for (int e = t; e < B * R1; e += NT) M[(e % B) * W + 2 * B + e / B] = blk[2 * BB + e];
  fetch(0);
  for (int i = 0; i < k; i++) {
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const int e = t + NT * u;
      if (e < BB) { M[(e % B) * W + B + e / B] = rO[u]; Dn[e] = rD[u]; }    // O_i^T
    }
#pragma unroll
    for (int u = 0; u < NG; u++) {
      const int e = t + NT * u;
      if (e < B * R1) Gn[e] = rG[u];
    }
    __syncthreads();
    if (i + 1 < k) fetch(i + 1);
    for (int j = 0; j < B; j++) {
      double piv = M[j * W + j];
      if (!(piv > 0.0)) { if (t == 0) *flag = 1; piv = 1.0; }
      const double pinv = 1.0 / piv, sinv = 1.0 / sqrt(piv);
      double v[NM];
#pragma unroll
      for (int u = 0; u < NM; u++) {
        const int e = t + NT * u;
        if (e < B * W) {
          const int r = e / W, c = e - r * W;
          const double m = M[e];
          if (r < j || c < j) v[u] = m;
          else if (r == j) v[u] = m * sinv;
          else v[u] = m - M[j * W + r] * M[j * W + c] * pinv;
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < NM; u++) {
        const int e = t + NT * u;
        if (e < B * W) M[e] = v[u];
      }
      __syncthreads();
    }
    double nS[NB], nG[NG];
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const int e = t + NT * u;
      if (e < BB) {
        const int r = e / B, c = e % B;
        double acc = Dn[e];
        for (int q = 0; q < B; q++) acc -= M[q * W + B + r] * M[q * W + B + c];
        nS[u] = acc;
      }
    }
#pragma unroll
    for (int u = 0; u < NG; u++) {
      const int e = t + NT * u;
      if (e < B * R1) {
        const int c = e / B, r = e - c * B;
        double acc = Gn[e];
        for (int q = 0; q < B; q++) acc -= M[q * W + B + r] * M[q * W + 2 * B + c];
        nG[u] = acc;
      }
    }
#pragma unroll
    for (int u = 0; u < NTT; u++) {
      const int e = t + NT * u;
      if (e < R1 * R1) {
        const int p = e / R1, c = e - p * R1;
        double acc = T[u];
        for (int q = 0; q < B; q++) acc += M[q * W + 2 * B + p] * M[q * W + 2 * B + c];
        T[u] = acc;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const int e = t + NT * u;
      if (e < BB) M[(e / B) * W + e % B] = nS[u];
    }
#pragma unroll
    for (int u = 0; u < NG; u++) {
      const int e = t + NT * u;
      if (e < B * R1) M[(e % B) * W + 2 * B + e / B] = nG[u];
    }
    __syncthreads();
  }
  for (int e = t; e < BB; e += NT) out[(e / B) * n + e % B] = M[(e / B) * W + e % B];
  for (int e = t; e < B * R1; e += NT) {
    const int c = e / B, r = e - c * B;
    const double m = M[r * W + 2 * B + c];
    if (c == 0) out[n * n + r] = m;
    else { out[r * n + B + c - 1] = m; out[(B + c - 1) * n + r] = m; }
  }
#pragma unroll
  for (int u = 0; u < NTT; u++) {
    const int e = t + NT * u;
    if (e < R1 * R1) {
      const int p = e / R1, c = e - p * R1;
      if (p >= 1 && c >= 1) out[(B + p - 1) * n + B + c - 1] = head[(p - 1) * nl + c - 1] - T[u];
      else if (p >= 1) out[n * n + B + p - 1] = head[nl * nl + p - 1] - T[u];
    }
  }
}

// ------------------------------------------------------------------ the states
// dst[r * dstride + doff + i] = src[r * sstride + soff + i], i < n: the SoA arrays move to their new stride on the device
__global__ void __launch_bounds__(256) k_move_states(const double *src, int sstride, int soff, double *dst, int dstride, int doff, int n, int rows) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long)rows * n) return;
  const int r = (int)(id / n), i = (int)(id - (long)r * n);
  dst[(size_t)r * dstride + doff + i] = src[(size_t)r * sstride + soff + i];
}
// dst[r * dstride + doff + i] = src[i * rows + r]: states in the caller's layout (one state after the other) into the SoA arrays
__global__ void __launch_bounds__(256) k_scatter_states(const double *src, double *dst, int dstride, int doff, int n, int rows) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long)rows * n) return;
  const int i = (int)(id / rows), r = (int)(id - (long)i * rows);
  dst[(size_t)r * dstride + doff + i] = src[id];
}
// out = [pose_i (pd) | vel_i (d)]
__global__ void __launch_bounds__(64) k_read_state(const double *pose, const double *vel, int stride, int i, int pd, int d, double *out) {
  const int t = threadIdx.x;
  if (t < pd) out[t] = pose[(size_t)t * stride + i];
  else if (t < pd + d) out[t] = vel[(size_t)(t - pd) * stride + i];
}

// what the four entry points ask of a handle
int fl_guard(gpslam_hip_handle *h, const char *who) {
  const char *why = nullptr;
  if (h->cfg.precision != GPSLAM_FP64) why = "an fp32 handle";
  else if (sharded(h)) why = "a sharded handle";
  else if (h->fs.split) why = "a piece of a split chain";
  else if (h->cfg.force_segmented == 1 || (h->compiled && h->fs.active)) why = "the segmented landmark path";
  if (!why) return 0;
  return fail(h, GPSLAM_E_UNSUPPORTED, (std::string(who) + ": not on " + why + " (fixed-lag smoothing runs on one fp64 handle with the dense landmark border)").c_str());
}

// Lambda = A^T A, A^T c = rhs: Cholesky with diagonal pivoting of the symmetrised Lambda; a pivot at or below thr ends it (the
// remaining rows of A are zero).  A: b x b row-major, c: b.
void factor_lambda(int b, const double *Lam, const double *rhs, double thr, double *A, double *c) {
  std::vector<double> Wk((size_t)b * b), L((size_t)b * b, 0.0);
  std::vector<int> perm(b);
  std::iota(perm.begin(), perm.end(), 0);
  for (int i = 0; i < b; i++)
    for (int j = 0; j < b; j++) Wk[i * b + j] = 0.5 * (Lam[i * b + j] + Lam[j * b + i]);
  int rank = 0;
  for (int j = 0; j < b; j++) {
    int p = j;
    for (int i = j + 1; i < b; i++) if (Wk[i * b + i] > Wk[p * b + p]) p = i;
    if (p != j) {
      std::swap(perm[j], perm[p]);
      for (int q = 0; q < b; q++) std::swap(Wk[j * b + q], Wk[p * b + q]);
      for (int q = 0; q < b; q++) std::swap(Wk[q * b + j], Wk[q * b + p]);
      for (int q = 0; q < j; q++) std::swap(L[j * b + q], L[p * b + q]);
    }
    const double piv = Wk[j * b + j];
    if (!(piv > thr)) break;
    const double ljj = std::sqrt(piv);
    L[j * b + j] = ljj;
    for (int i = j + 1; i < b; i++) L[i * b + j] = Wk[i * b + j] / ljj;
    for (int i = j + 1; i < b; i++)
      for (int m = j + 1; m < b; m++) Wk[i * b + m] -= L[i * b + j] * L[m * b + j];
    rank = j + 1;
  }
  std::fill(A, A + (size_t)b * b, 0.0);
  std::fill(c, c + b, 0.0);
  for (int i = 0; i < rank; i++) {
    for (int m = i; m < b; m++) A[i * b + perm[m]] = L[m * b + i];
    double s = rhs[perm[i]];
    for (int q = 0; q < i; q++) s -= L[i * b + q] * c[q];
    c[i] = s / L[i * b + i];
  }
}

// keeps the entries of a per-factor array (w values per factor) whose factor stays; an empty array is an optional table that is
// not in use, any other size was checked by widths_ok before the handle changed
template <typename V> void keep_of(std::vector<V> &v, const std::vector<char> &keep, size_t w) {
  if (v.empty()) return;
  size_t o = 0;
  for (size_t f = 0; f < keep.size(); f++)
    if (keep[f]) { if (o != f) std::copy(v.begin() + f * w, v.begin() + (f + 1) * w, v.begin() + o * w); o++; }
  v.resize(o * w);
}
std::vector<char> keep_mask(const std::vector<int32_t> &idx, int k) {
  std::vector<char> m(idx.size());
  for (size_t f = 0; f < idx.size(); f++) m[f] = idx[f] >= k;
  return m;
}
void shift_idx(std::vector<int32_t> &idx, int k) { for (int32_t &i : idx) i -= k; }

// every per-factor array of the handle that follows a state index: fn(array, the index array of its factors, values per factor, name).
// The index arrays themselves are not listed: marginalize_head filters them last.
template <typename F> void each_factor_array(gpslam_hip_handle *h, F fn) {
  const size_t d = (size_t)h->d, b = (size_t)h->b, pd = (size_t)h->pd;
  fn(h->gp_dt, h->gp_left, (size_t)1, "gp_dt");
  fn(h->gp_q, h->gp_left, (size_t)1, "gp_q");
  for (SimpleSet *s : {&h->pri, &h->vpri, &h->btw}) {
    fn(s->meas, s->idx, (size_t)s->width, "meas of a prior / between set");
    fn(s->sig, s->idx, d, "sigmas of a prior / between set");
  }
  for (MeasSet &s : h->ms) {
    fn(s.lm, s.idx, (size_t)1, "lm");
    fn(s.meas, s.idx, (size_t)s.mw, "meas of a measurement set");
    fn(s.sig, s.idx, (size_t)s.rows, "sigmas of a measurement set");
    fn(s.dt, s.idx, (size_t)1, "dt");
    fn(s.tau, s.idx, (size_t)1, "tau");
    fn(s.aidx, s.idx, (size_t)1, "aidx");
    fn(s.sqi, s.idx, (size_t)s.rows * s.rows, "sqi");
    fn(s.rob, s.idx, (size_t)2, "rob");
  }
  fn(h->sg.lin, h->sg.idx, pd + d, "lin of the state Gaussians");
  fn(h->sg.A, h->sg.idx, b * b, "A of the state Gaussians");
  fn(h->sg.c, h->sg.idx, b, "c of the state Gaussians");
  const size_t n = b + (size_t)h->bg.nl;
  fn(h->bg.lin, h->bg.idx, pd + d + (size_t)h->bg.nl, "lin of the border Gaussians");
  fn(h->bg.A, h->bg.idx, n * n, "A of the border Gaussians");
  fn(h->bg.c, h->bg.idx, n, "c of the border Gaussians");
}
// an array is empty (an optional table that is not in use) or holds w values per factor; anything else is a mistake of this library
const char *widths_ok(gpslam_hip_handle *h) {
  const char *bad = nullptr;
  each_factor_array(h, [&](auto &v, const std::vector<int32_t> &idx, size_t w, const char *name) {
    if (!bad && !v.empty() && v.size() != idx.size() * w) bad = name;
  });
  return bad;
}

const char *kMeasNames[kNumMeasKinds] = {"interpolated range", "range", "interpolated attitude", "interpolated GPS", "odometry2d", "bearing-range",
                                         "interpolated projection", "AHRS"};

}  // namespace

// ---- what compile() and the factor launches call (api_common.hpp)
int state_gauss_upload(gpslam_hip_handle *h, const std::vector<int> &row0) {
  StateGauss &s = h->sg;
  int rc;
  if ((rc = upload(h, s.d_idx, s.idx)) || (rc = upload(h, s.d_lin, s.lin)) || (rc = upload(h, s.d_A, s.A)) || (rc = upload(h, s.d_c, s.c))) return rc;
  return upload(h, s.d_row0, row0);
}

void state_gauss_eval(gpslam_hip_handle *h, int pass, double *partial, hipStream_t st) {
  const StateGauss &s = h->sg;
  SgArgs a;
  a.pose = h->pose.as<double>(); a.vel = h->vel.as<double>(); a.stride = h->stride; a.count = s.count(); a.chart = h->cfg.chart;
  a.idx = s.d_idx.as<int>(); a.row0 = s.d_row0.as<int>();
  a.lin = s.d_lin.as<double>(); a.A = s.d_A.as<double>(); a.c = s.d_c.as<double>();
  a.rowLR = h->rowLR.as<double>(); a.rowE = h->rowE.as<double>(); a.partial = partial;
  const int nb = nblocks(a.count, 128);
  dispatch_mf(h->mf, [&](auto tag) {
    constexpr int MF = decltype(tag)::value;
    if (pass == 0) k_state_gauss<MF, true><<<dim3(nb), dim3(128), 0, st>>>(a);
    else k_state_gauss<MF, false><<<dim3(nb), dim3(128), 0, st>>>(a);
  });
}

int border_gauss_upload(gpslam_hip_handle *h) {
  BorderGauss &s = h->bg;
  int rc;
  if ((rc = upload(h, s.d_idx, s.idx)) || (rc = upload(h, s.d_lin, s.lin)) || (rc = upload(h, s.d_A, s.A)) || (rc = upload(h, s.d_c, s.c))) return rc;
  HIPCHK(s.d_r.reserve((size_t)s.count() * (h->b + s.nl) * sizeof(double)));
  return 0;
}

void border_gauss_eval(gpslam_hip_handle *h, int pass, double *partial, hipStream_t st) {
  const BorderGauss &s = h->bg;
  BgArgs a;
  a.pose = h->pose.as<double>(); a.vel = h->vel.as<double>(); a.lmk = h->lmk.as<double>();
  a.stride = h->stride; a.count = s.count(); a.chart = h->cfg.chart; a.nl = s.nl;
  a.idx = s.d_idx.as<int>(); a.lin = s.d_lin.as<double>(); a.A = s.d_A.as<double>(); a.c = s.d_c.as<double>();
  a.r = s.d_r.as<double>(); a.partial = partial;
  dispatch_mf(h->mf, [&](auto tag) {
    constexpr int MF = decltype(tag)::value;
    if (pass == 0) k_border_gauss<MF, true><<<dim3(1), dim3(64), 0, st>>>(a);
    else k_border_gauss<MF, false><<<dim3(1), dim3(64), 0, st>>>(a);
  });
}

namespace {
BgPatchArgs bg_patch_args(gpslam_hip_handle *h) {
  const BorderGauss &s = h->bg;
  BgPatchArgs a;
  a.count = s.count(); a.nl = s.nl; a.B = h->b; a.R = h->R;
  a.idx = s.d_idx.as<int>(); a.A = s.d_A.as<double>(); a.r = s.d_r.as<double>();
  a.blk = h->lv[0].blk.as<double>(); a.gsave = nullptr;
  a.x = h->lv[0].x.as<double>();
  a.S = h->lm_S.as<double>(); a.gL = h->lm_S.as<double>() + (size_t)h->nl * h->R;
  return a;
}
}  // namespace

void border_gauss_inject(gpslam_hip_handle *h, bool save_g) {
  BgPatchArgs a = bg_patch_args(h);
  a.gsave = save_g ? h->gsave.as<double>() : nullptr;
  k_border_inject<<<dim3(1), dim3(256), 0, h->stream>>>(a);
}

void border_gauss_schur(gpslam_hip_handle *h) {
  const BgPatchArgs a = bg_patch_args(h);
  k_border_schur<<<dim3(nblocks(a.nl * a.R, 256)), dim3(256), 0, h->stream>>>(a);
}

extern "C" {

int gpslam_hip_add_border_gaussians(gpslam_hip_handle *h, int32_t count, const int32_t *idx, const double *pose_lin, const double *vel_lin,
                                    const double *lm_lin, const double *A, const double *c) {
  if (!h || count < 0 || (count > 0 && (!idx || !pose_lin || !vel_lin || !lm_lin || !A || !c))) return GPSLAM_E_INVALID;
  int rc = fl_guard(h, "add_border_gaussians");
  if (rc) return rc;
  const int pd = h->pd, d = h->d, b = h->b, nl = h->L * h->ld, n = b + nl;
  if (nl <= 0) return fail(h, GPSLAM_E_INVALID, "add_border_gaussians: the handle has no landmarks (set_landmarks first; add_state_gaussians is the factor on a state alone)");
  BorderGauss &s = h->bg;
  if (s.count() > 0 && s.nl != nl) return fail(h, GPSLAM_E_INVALID, "add_border_gaussians: the stored border Gaussians span another number of landmarks (set_landmarks changed it)");
  for (int f = 0; f < count; f++)
    if (idx[f] < 0 || idx[f] >= h->N) return fail(h, GPSLAM_E_INVALID, "factor index out of range");
  auto finite = [](const double *v, size_t m) { for (size_t q = 0; q < m; q++) if (!std::isfinite(v[q])) return false; return true; };
  if (!finite(A, (size_t)count * n * n)) return fail(h, GPSLAM_E_INVALID, "add_border_gaussians: A must be finite");
  if (!finite(c, (size_t)count * n)) return fail(h, GPSLAM_E_INVALID, "add_border_gaussians: c must be finite");
  if (!finite(pose_lin, (size_t)count * pd)) return fail(h, GPSLAM_E_INVALID, "add_border_gaussians: pose_lin must be finite");
  if (!finite(vel_lin, (size_t)count * d)) return fail(h, GPSLAM_E_INVALID, "add_border_gaussians: vel_lin must be finite");
  if (!finite(lm_lin, (size_t)count * nl)) return fail(h, GPSLAM_E_INVALID, "add_border_gaussians: lm_lin must be finite");
  if (count == 0) return 0;
  s.nl = nl;
  s.idx.insert(s.idx.end(), idx, idx + count);
  for (int f = 0; f < count; f++) {
    s.lin.insert(s.lin.end(), pose_lin + (size_t)f * pd, pose_lin + (size_t)(f + 1) * pd);
    s.lin.insert(s.lin.end(), vel_lin + (size_t)f * d, vel_lin + (size_t)(f + 1) * d);
    s.lin.insert(s.lin.end(), lm_lin + (size_t)f * nl, lm_lin + (size_t)(f + 1) * nl);
  }
  s.A.insert(s.A.end(), A, A + (size_t)count * n * n);
  s.c.insert(s.c.end(), c, c + (size_t)count * n);
  h->compiled = false;
  h->mg.invalidate();
  return 0;
}

int gpslam_hip_get_border_gaussians(gpslam_hip_handle *h, int32_t *idx, double *pose_lin, double *vel_lin, double *lm_lin, double *A, double *c) {
  if (!h) return GPSLAM_E_INVALID;
  const BorderGauss &s = h->bg;
  const int m = s.count(), pd = h->pd, d = h->d, nl = s.nl, w = pd + d + nl;
  if (m > 0 && nl != h->L * h->ld && (lm_lin || A || c))   // (a caller sizes its arrays from the handle's landmarks)
    return fail(h, GPSLAM_E_INVALID, "get_border_gaussians: the stored border Gaussians span another number of landmarks than the handle has (set_landmarks changed it)");
  for (int f = 0; f < m; f++) {
    if (idx) idx[f] = s.idx[f];
    if (pose_lin) std::memcpy(pose_lin + (size_t)f * pd, &s.lin[(size_t)f * w], sizeof(double) * pd);
    if (vel_lin) std::memcpy(vel_lin + (size_t)f * d, &s.lin[(size_t)f * w + pd], sizeof(double) * d);
    if (lm_lin) std::memcpy(lm_lin + (size_t)f * nl, &s.lin[(size_t)f * w + pd + d], sizeof(double) * nl);
  }
  if (A && m > 0) std::memcpy(A, s.A.data(), sizeof(double) * s.A.size());
  if (c && m > 0) std::memcpy(c, s.c.data(), sizeof(double) * s.c.size());
  return m;
}

int gpslam_hip_marginalize_head_onto_landmarks(gpslam_hip_handle *h, int32_t enable) {
  if (!h) return GPSLAM_E_INVALID;
  h->fl_onto_lm = enable != 0;
  return 0;
}

int gpslam_hip_get_head_prior_border(gpslam_hip_handle *h, double *lm_lin, double *Lambda, double *gamma) {
  if (!h) return GPSLAM_E_INVALID;
  if (h->hpb.empty()) return fail(h, GPSLAM_E_INVALID, "get_head_prior_border: the last gpslam_hip_marginalize_head on this handle, if any, was not one onto the landmarks");
  const int nl = h->hpb_nl, n = h->b + nl;
  if (nl != h->L * h->ld && (lm_lin || Lambda || gamma))   // (a caller sizes its arrays from the handle's landmarks)
    return fail(h, GPSLAM_E_INVALID, "get_head_prior_border: the head prior spans another number of landmarks than the handle has now (set_landmarks changed it)");
  const double *p = h->hpb.data();
  if (lm_lin) std::memcpy(lm_lin, p, sizeof(double) * nl);
  if (Lambda) std::memcpy(Lambda, p + nl, sizeof(double) * n * n);
  if (gamma) std::memcpy(gamma, p + nl + (size_t)n * n, sizeof(double) * n);
  return 0;
}

int gpslam_hip_add_state_gaussians(gpslam_hip_handle *h, int32_t count, const int32_t *idx, const double *pose_lin, const double *vel_lin,
                                   const double *A, const double *c) {
  if (!h || count < 0 || (count > 0 && (!idx || !pose_lin || !vel_lin || !A || !c))) return GPSLAM_E_INVALID;
  int rc = fl_guard(h, "add_state_gaussians");
  if (rc) return rc;
  const int pd = h->pd, d = h->d, b = h->b;
  for (int f = 0; f < count; f++)
    if (idx[f] < 0 || idx[f] >= h->N) return fail(h, GPSLAM_E_INVALID, "factor index out of range");
  for (size_t q = 0; q < (size_t)count * b * b; q++)
    if (!std::isfinite(A[q])) return fail(h, GPSLAM_E_INVALID, "add_state_gaussians: A must be finite");
  for (size_t q = 0; q < (size_t)count * b; q++)
    if (!std::isfinite(c[q])) return fail(h, GPSLAM_E_INVALID, "add_state_gaussians: c must be finite");
  for (size_t q = 0; q < (size_t)count * pd; q++)
    if (!std::isfinite(pose_lin[q])) return fail(h, GPSLAM_E_INVALID, "add_state_gaussians: pose_lin must be finite");
  for (size_t q = 0; q < (size_t)count * d; q++)
    if (!std::isfinite(vel_lin[q])) return fail(h, GPSLAM_E_INVALID, "add_state_gaussians: vel_lin must be finite");
  StateGauss &s = h->sg;
  s.idx.insert(s.idx.end(), idx, idx + count);
  for (int f = 0; f < count; f++) {
    s.lin.insert(s.lin.end(), pose_lin + (size_t)f * pd, pose_lin + (size_t)(f + 1) * pd);
    s.lin.insert(s.lin.end(), vel_lin + (size_t)f * d, vel_lin + (size_t)(f + 1) * d);
  }
  s.A.insert(s.A.end(), A, A + (size_t)count * b * b);
  s.c.insert(s.c.end(), c, c + (size_t)count * b);
  h->compiled = false;
  h->mg.invalidate();
  return 0;
}

int gpslam_hip_get_state_gaussians(gpslam_hip_handle *h, int32_t *idx, double *pose_lin, double *vel_lin, double *A, double *c) {
  if (!h) return GPSLAM_E_INVALID;
  const StateGauss &s = h->sg;
  const int n = s.count(), pd = h->pd, d = h->d, b = h->b;
  for (int f = 0; f < n; f++) {
    if (idx) idx[f] = s.idx[f];
    if (pose_lin) std::memcpy(pose_lin + (size_t)f * pd, &s.lin[(size_t)f * (pd + d)], sizeof(double) * pd);
    if (vel_lin) std::memcpy(vel_lin + (size_t)f * d, &s.lin[(size_t)f * (pd + d) + pd], sizeof(double) * d);
  }
  if (A && n > 0) std::memcpy(A, s.A.data(), sizeof(double) * s.A.size());
  if (c && n > 0) std::memcpy(c, s.c.data(), sizeof(double) * s.c.size());
  return n;
}

int gpslam_hip_marginalize_head(gpslam_hip_handle *h, int32_t k) {
  if (!h) return GPSLAM_E_INVALID;
  int rc = fl_guard(h, "marginalize_head");
  if (rc) return rc;
  if (h->mf == ROT3_BIAS) return fail(h, GPSLAM_E_UNSUPPORTED, "marginalize_head: not on a GPSLAM_ROT3_BIAS handle (the pad coordinates of its velocity slot)");
  if ((rc = need_local(h))) return rc;
  const int N = h->N, b = h->b, pd = h->pd, d = h->d;
  if (k < 1 || k >= N) return fail(h, GPSLAM_E_INVALID, "marginalize_head: 1 <= k <= N - 1");
  // onto the landmarks (gpslam_hip_marginalize_head_onto_landmarks): the prior spans the oldest kept state and every landmark
  // (block size 4, the 2-D linear chain: no factor of that manifold names a landmark, the state prior is the whole marginal)
  const bool joint = h->fl_onto_lm && h->nl > 0 && b != 4;
  if (joint && h->clo.P > 1)
    return fail(h, GPSLAM_E_UNSUPPORTED, "marginalize_head onto the landmarks: not with loop closures in column passes (set_closure_passes): the border Gaussian it leaves is refused there");
  for (int fk = 0; fk < kNumMeasKinds && !joint; fk++) {
    const MeasSet &s = h->ms[fk];
    if (!s.haslm) continue;
    for (int f = 0; f < s.count(); f++)
      if (s.idx[f] < k)
        return fail(h, GPSLAM_E_UNSUPPORTED, (std::string("marginalize_head: ") + kMeasNames[fk] + " factor " + std::to_string(f) + " (state " + std::to_string(s.idx[f]) +
                                              ") is in the head and names landmark " + std::to_string(s.lm[f]) + ": the prior would span the state and that landmark").c_str());
  }
  for (int f = 0; f < h->bg.count() && !joint; f++)
    if (h->bg.idx[f] < k)
      return fail(h, GPSLAM_E_UNSUPPORTED, ("marginalize_head: border Gaussian " + std::to_string(f) + " (state " + std::to_string(h->bg.idx[f]) +
                                            ") is in the head and spans the landmarks: gpslam_hip_marginalize_head_onto_landmarks").c_str());
  for (int f = 0; f < h->clo.fac.count(); f++)
    if (h->clo.fac.idx[f] < k || h->clo.second[f] < k)
      return fail(h, GPSLAM_E_UNSUPPORTED, ("marginalize_head: loop closure " + std::to_string(f) + " (" + std::to_string(h->clo.fac.idx[f]) + ", " + std::to_string(h->clo.second[f]) +
                                            ") reaches into the head").c_str());
  if (const char *bad = widths_ok(h))
    return fail(h, GPSLAM_E_INVALID, (std::string("marginalize_head: internal error: the per-factor array ") + bad + " does not hold its width per factor").c_str());
  // ---- the head's linearisation: the handle's own rows and records (lambda = 0, robust weights), then the recursion
  LaunchMode rows;
  rows.d3_rows = true;   // the d = 3 GP priors as rows: the head's share of block k is summed from the tables, so they hold every row
  if ((rc = impl64::launch_factors(h, rows, 0, 0)) || (rc = impl64::launch_assemble(h, rows, false))) return rc;
  const int BB = b * b, nl = joint ? h->nl : 0, R1 = 1 + nl, n = b + nl;
  // [D_k^left | g_k^left | B_k^left] (k_head_left, k_head_left_lm), [Lambda (n x n) | g' (n)], [pose_k | vel_k], the landmarks
  const int nleft = BB + b * R1, nout = nleft + n * n + n + pd + d + nl, nhead = nl * nl + nl;
  HIPCHK(h->fl_out.reserve((size_t)nout * sizeof(double)));
  HIPCHK(h->fl_flag.reserve(sizeof(int)));
  HIPCHK(hipMemsetAsync(h->fl_flag.p, 0, sizeof(int), h->stream));
  double *left = h->fl_out.as<double>(), *out = left + nleft, *state = out + n * n + n;
  const int BS = 2 * BB + b * h->R;
  if (joint) {
    HIPCHK(h->fl_head.reserve((size_t)nhead * sizeof(double)));
    k_head_left_lm<<<dim3(1), dim3(256), 0, h->stream>>>(h->rowptr.as<int>(), h->rowLR.as<double>(), h->rowM.as<double>(), h->rowLm.as<int>(), b, h->ld, nl, k, left);
    k_head_sums<<<dim3(nblocks(nhead, 256)), dim3(256), 0, h->stream>>>(h->rowptr.as<int>(), h->rowM.as<double>(), h->rowE.as<double>(), h->rowLm.as<int>(), h->ld, nl, k, b,
                                                                          h->bg.count(), h->bg.d_idx.as<int>(), h->bg.d_A.as<double>(), h->bg.d_r.as<double>(),
                                                                          h->fl_head.as<double>());
    HIPCHK(hipMemcpyAsync(state + pd + d, h->lmk.p, (size_t)nl * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  }
  dispatch_b(b, [&](auto tag) {
    constexpr int B = decltype(tag)::value;
    k_head_left<B><<<dim3(1), dim3(64), 0, h->stream>>>(h->rowptr.as<int>(), h->rowLR.as<double>(), h->rowE.as<double>(), h->crowptr.as<int>(), h->rowC.as<double>(),
                                                         h->rowCE.as<double>(), k, left);
    if constexpr (B != 4) {
      if (joint) { k_head_schur_border<B><<<dim3(1), dim3(256), 0, h->stream>>>(h->lv[0].blk.as<double>(), BS, k, nl, left, h->fl_head.as<double>(), out, h->fl_flag.as<int>()); return; }
    }
    k_head_schur<B><<<dim3(1), dim3(64), 0, h->stream>>>(h->lv[0].blk.as<double>(), BS, k, left, out, h->fl_flag.as<int>());
  });
  k_read_state<<<dim3(1), dim3(64), 0, h->stream>>>(h->pose.as<double>(), h->vel.as<double>(), h->stride, k, pd, d, state);
  HIPCHK(hipGetLastError());
  std::vector<double> host(nout), hhead(nhead);
  int flag = 0;
  HIPCHK(hipMemcpyAsync(host.data(), h->fl_out.p, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (joint) HIPCHK(hipMemcpyAsync(hhead.data(), h->fl_head.p, (size_t)nhead * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&flag, h->fl_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (flag) return fail(h, GPSLAM_E_NOT_SPD, "marginalize_head: a pivot block of the head is not positive definite (nothing in the head determines one of its states)");
  const double *Dl = host.data(), *Lam = host.data() + nleft, *gk = Lam + n * n, *st = gk + n;
  for (int q = 0; q < n * n + n; q++)
    if (!std::isfinite(Lam[q])) return fail(h, GPSLAM_E_NAN, "marginalize_head: the head's linearisation is not finite");
  // the pivot threshold: n eps max|diag| of the head's own share of [D_k^left ; H_LL^head], before the subtraction
  double scale = 0.0;
  for (int q = 0; q < b; q++) scale = std::max(scale, std::fabs(Dl[q * b + q]));
  for (int q = 0; q < nl; q++) scale = std::max(scale, std::fabs(hhead[(size_t)q * nl + q]));
  std::vector<double> A((size_t)n * n), c((size_t)n);
  factor_lambda(n, Lam, gk, n * DBL_EPSILON * scale, A.data(), c.data());   // (g'_k = -gamma: the records hold -J^T e)
  // ---- the new states, on the device, into the handle's second state buffer (the one Levenberg-Marquardt keeps its backup in: free
  // between calls); the two buffers then change places.  Nothing of the handle has changed up to here
  const int N2 = N - k, stride2 = N2 + 1;
  HIPCHK(h->pose_bak.reserve((size_t)pd * stride2 * sizeof(double)));
  HIPCHK(h->vel_bak.reserve((size_t)d * stride2 * sizeof(double)));
  // (N2 + 1 entries: the halo slot behind the last state moves along)
  k_move_states<<<dim3(nblocks(pd * stride2, 256)), dim3(256), 0, h->stream>>>(h->pose.as<double>(), h->stride, k, h->pose_bak.as<double>(), stride2, 0, stride2, pd);
  k_move_states<<<dim3(nblocks(d * stride2, 256)), dim3(256), 0, h->stream>>>(h->vel.as<double>(), h->stride, k, h->vel_bak.as<double>(), stride2, 0, stride2, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  std::swap(h->pose, h->pose_bak);
  std::swap(h->vel, h->vel_bak);
  h->N = N2; h->stride = stride2;
  // ---- the factors: the head's go, the others move down by k
  each_factor_array(h, [&](auto &v, const std::vector<int32_t> &idx, size_t w, const char *) { keep_of(v, keep_mask(idx, k), w); });
  std::vector<std::vector<int32_t> *> index_arrays = {&h->gp_left, &h->pri.idx, &h->vpri.idx, &h->btw.idx, &h->sg.idx, &h->bg.idx};
  for (MeasSet &s : h->ms) index_arrays.push_back(&s.idx);
  for (std::vector<int32_t> *idx : index_arrays) {
    keep_of(*idx, keep_mask(*idx, k), 1);
    shift_idx(*idx, k);
  }
  shift_idx(h->clo.fac.idx, k);
  shift_idx(h->clo.second, k);
  if (joint) {
    BorderGauss &s = h->bg;
    s.nl = nl;
    s.idx.push_back(0);
    s.lin.insert(s.lin.end(), st, st + pd + d + nl);
    s.A.insert(s.A.end(), A.begin(), A.end());
    s.c.insert(s.c.end(), c.begin(), c.end());
  } else {
    StateGauss &s = h->sg;
    s.idx.push_back(0);
    s.lin.insert(s.lin.end(), st, st + pd + d);
    s.A.insert(s.A.end(), A.begin(), A.end());
    s.c.insert(s.c.end(), c.begin(), c.end());
  }
  // get_head_prior: the state block of Lambda and gamma, so its sizes never change; get_head_prior_border: all of it
  h->hp.assign(st, st + pd + d);
  for (int r = 0; r < b; r++) h->hp.insert(h->hp.end(), Lam + (size_t)r * n, Lam + (size_t)r * n + b);
  for (int q = 0; q < b; q++) h->hp.push_back(-gk[q]);
  h->hpb.clear();
  h->hpb_nl = nl;
  if (joint) {
    h->hpb.assign(st + pd + d, st + pd + d + nl);
    h->hpb.insert(h->hpb.end(), Lam, Lam + (size_t)n * n);
    for (int q = 0; q < n; q++) h->hpb.push_back(-gk[q]);
  }
  h->defer.clear();
  h->compiled = false;
  h->mg.invalidate();
  return 0;
}

int gpslam_hip_get_head_prior(gpslam_hip_handle *h, double *pose_lin, double *vel_lin, double *Lambda, double *gamma) {
  if (!h) return GPSLAM_E_INVALID;
  if (h->hp.empty()) return fail(h, GPSLAM_E_INVALID, "get_head_prior: no successful gpslam_hip_marginalize_head on this handle yet");
  const int pd = h->pd, d = h->d, b = h->b;
  const double *p = h->hp.data();
  if (pose_lin) std::memcpy(pose_lin, p, sizeof(double) * pd);
  if (vel_lin) std::memcpy(vel_lin, p + pd, sizeof(double) * d);
  if (Lambda) std::memcpy(Lambda, p + pd + d, sizeof(double) * b * b);
  if (gamma) std::memcpy(gamma, p + pd + d + b * b, sizeof(double) * b);
  return 0;
}

int gpslam_hip_append_states(gpslam_hip_handle *h, int32_t n, const double *pose, const double *vel) {
  if (!h || n < 0 || (n > 0 && (!pose || !vel))) return GPSLAM_E_INVALID;
  int rc = fl_guard(h, "append_states");
  if (rc) return rc;
  if (h->N <= 0 || !h->pose.p) return fail(h, GPSLAM_E_INVALID, "append_states: set_states() first");
  if (n == 0) return 0;
  (void)hipSetDevice(h->cfg.device);
  const int N = h->N, pd = h->pd, d = h->d, N2 = N + n, stride2 = N2 + 1;
  DevBuf in_pose, in_vel, pose2, vel2;   // (a failure below frees all four on the way out)
  HIPCHK(in_pose.reserve((size_t)n * pd * sizeof(double)));
  HIPCHK(in_vel.reserve((size_t)n * d * sizeof(double)));
  HIPCHK(pose2.reserve((size_t)pd * stride2 * sizeof(double)));
  HIPCHK(vel2.reserve((size_t)d * stride2 * sizeof(double)));
  HIPCHK(hipMemcpyAsync(in_pose.p, pose, (size_t)n * pd * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(in_vel.p, vel, (size_t)n * d * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(pose2.p, 0, (size_t)pd * stride2 * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(vel2.p, 0, (size_t)d * stride2 * sizeof(double), h->stream));
  k_move_states<<<dim3(nblocks(pd * N, 256)), dim3(256), 0, h->stream>>>(h->pose.as<double>(), h->stride, 0, pose2.as<double>(), stride2, 0, N, pd);
  k_move_states<<<dim3(nblocks(d * N, 256)), dim3(256), 0, h->stream>>>(h->vel.as<double>(), h->stride, 0, vel2.as<double>(), stride2, 0, N, d);
  k_scatter_states<<<dim3(nblocks(pd * n, 256)), dim3(256), 0, h->stream>>>(in_pose.as<double>(), pose2.as<double>(), stride2, N, n, pd);
  k_scatter_states<<<dim3(nblocks(d * n, 256)), dim3(256), 0, h->stream>>>(in_vel.as<double>(), vel2.as<double>(), stride2, N, n, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  h->pose = std::move(pose2);
  h->vel = std::move(vel2);
  h->N = N2; h->stride = stride2;
  h->compiled = false;
  h->mg.invalidate();
  return 0;
}

}  // extern "C"
