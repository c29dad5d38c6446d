// closures.hpp -- the kernels of the loop closures (gpslam_hip_add_between_pairs).  fp64 only: compile() refuses closures on an fp32
// handle, and closures.hip, which launches them, is compiled once.  The marginals (marginals.hip, marginals_clo.hip) read the
// record layout (kCloLen) and the helpers clo_row_dot / clo_sym_entry from here.
#pragma once

#include "kernels.hpp"

namespace gps {

// ------------------------------------------------------------------ loop closures (round 6)
// gtsam::BetweenFactor<Pose>(x_i, x_j, measured) between NON-adjacent states: the one factor of a SLAM graph that leaves the chain
// (the reference's factors take arbitrary keys the same way, gpslam/gp/GaussianProcessPriorPose3.h:43-47).  Its whitened rows
// U = [.. A_i .. A_j ..] (d x N b, pose columns of two states) make the normal equations H0 + U^T U with H0 the block-tridiagonal
// (+ landmark border) matrix of everything else.  The chain solver stays what it is: the d columns of U^T ride through it as extra
// right-hand sides behind the landmark columns (Z = H0^-1 U^T), and
//   (H0 + U^T U)^-1 [g + U^T r | B] = X + Z Y,   X = H0^-1 [g | B],   Y = (I + U Z)^-1 ([r | 0] - U X),   r = -(whitened error)
// (Sherman-Morrison-Woodbury; I + U Z is d K x d K, symmetric positive definite) corrects the solution column AND the landmark
// columns before the landmark Schur complement is formed, so that landmarks and closures mix freely.  K closures cost K d of the
// kMaxRhs - 1 border columns.  Four small kernels: evaluate, inject the columns into the level-0 records, solve, correct.
struct CloArgs {
  const double *pose;     // SoA states
  int stride, count, chart;
  const int *first, *second;
  const double *meas, *sig;   // count x pose_dim, count x d
  const double *rob = nullptr;   // noiseModel::Robust (gpslam_hip_set_between_pairs_robust): count x 2 = (loss, k), or null
  double *out_w = nullptr;       // count: the weights w(r) (gpslam_hip_get_between_pairs_weights), or null
  double *A;              // count records [A_i (d x d) | A_j (d x d) | r (d)]: whitened H1, H2 and right-hand side
  double *partial;        // the closures' 0.5 |R e|^2 (one value)
  double *blk;            // level-0 block records [D | O | G (B x R)]
  int BS, B, R, col0;     // record length, block size, right-hand sides, first closure column (1 + nl)
  double *gsave;          // Levenberg-Marquardt: the gradient copy takes U^T r as well, or null
  double *x;              // level-0 solutions N x R x B
  int N, ncols;           // columns 0 .. ncols - 1 (the update and the landmark columns) are corrected
  double *Y;              // nc x ncols
  int *flag;
};
constexpr int kCloLen(int d) { return 2 * d * d + d; }

// Two expressions the closure kernels and the marginals' (marginals.hip, marginals_clo.hip) share, each written once.  A kernel
// takes one only where its code bytes stay what they were; the kernels that spell the expression out say which helper they mirror.
// (U x)[p][xc]: row p = k d + q of U -- row q of closure k's record A -- against column xc of the level-0 solution x (N x R x B) at
// the closure's two states: A_i against x_i first, then A_j against x_j, into one accumulator
template <int d> __device__ __forceinline__ double clo_row_dot(const double *A, const int *first, const int *second, const double *x, int R, int B, int p, int xc) {
  const int k = p / d, q = p - k * d;
  const double *rec = A + (size_t)k * kCloLen(d);
  const double *xi = x + ((size_t)first[k] * R + xc) * B, *xj = x + ((size_t)second[k] * R + xc) * B;
  double acc = 0.0;
  for (int m = 0; m < d; m++) acc += rec[q * d + m] * xi[m];
  for (int m = 0; m < d; m++) acc += rec[d * d + q * d + m] * xj[m];
  return acc;
}
// (I + 1/2 (U Z + (U Z)^T))[i][j] from (U Z)[i][j] and (U Z)[j][i]; diag: i == j
__device__ __forceinline__ double clo_sym_entry(bool diag, double uz_ij, double uz_ji) { return (diag ? 1.0 : 0.0) + 0.5 * (uz_ij + uz_ji); }

template <int MF, bool JAC> __global__ void __launch_bounds__(128) k_clo_eval(CloArgs a) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd;
  double err = 0.0;
  for (int f = threadIdx.x; f < a.count; f += 128) {
    const int i = a.first[f], j = a.second[f];
    double x1[pd], x2[pd], m[pd], e[d], H1[JAC ? d * d : 1], H2[JAC ? d * d : 1];
#pragma unroll
    for (int k = 0; k < pd; k++) {
      x1[k] = a.pose[(size_t)k * a.stride + i];
      x2[k] = a.pose[(size_t)k * a.stride + j];
      m[k] = a.meas[(size_t)f * pd + k];
    }
    PoseFactors<double, MF, JAC>::between(m, x1, x2, a.chart, e, H1, H2);
    double *rec = a.A + (size_t)f * kCloLen(d);
    // noiseModel::Robust, as in k_meas: both blocks and r scaled by sqrt(w(|whitened error|)), the cost takes rho
    bool robust = false;
    double sw = 1.0;
    if (a.rob) {
      const int loss = (int)a.rob[2 * (size_t)f];
      double wr = 1.0;
      if (loss != ROBUST_NONE) {
        double r2 = 0.0, rho;
#pragma unroll
        for (int r = 0; r < d; r++) {
          const double we = (1.0 / a.sig[(size_t)f * d + r]) * e[r];
          r2 += we * we;
        }
        robust_eval(loss, a.rob[2 * (size_t)f + 1], sqrt(r2), wr, rho);
        robust = true;
        sw = sqrt(wr);
        err += 2.0 * rho;
      }
      if (a.out_w) a.out_w[f] = wr;
    }
#pragma unroll
    for (int r = 0; r < d; r++) {
      double w = 1.0 / a.sig[(size_t)f * d + r];
      double we = w * e[r];
      if (robust) { w *= sw; we *= sw; }
      else err += we * we;
      if (JAC) {
#pragma unroll
        for (int c = 0; c < d; c++) { rec[r * d + c] = w * H1[r * d + c]; rec[d * d + r * d + c] = w * H2[r * d + c]; }
        rec[2 * d * d + r] = -we;
      }
    }
  }
  const double tot = block_sum(0.5 * err);
  if (threadIdx.x == 0) a.partial[0] = tot;
}

// the columns of U^T into the records of the two states of every closure (k_assemble_ghost left those columns zero); one workgroup.
// [k0, k1): the closures whose columns ride in this pass, in columns col0 .. col0 + (k1 - k0) d - 1 (one pass: all of them); the
// gradient copy takes U^T r of EVERY closure whenever it is asked for.
template <int d> __global__ void __launch_bounds__(256) k_clo_inject(CloArgs a, int k0, int k1) {
  const int per = 2 * d * d;
  for (int t = threadIdx.x; t < (k1 - k0) * per; t += 256) {
    const int kk = t / per, u = t - kk * per, k = k0 + kk;
    const int side = u / (d * d), v = u - side * d * d;
    const int q = v / d, c = v - q * d;
    const int s = side ? a.second[k] : a.first[k];
    a.blk[(size_t)s * a.BS + 2 * a.B * a.B + (size_t)(a.col0 + kk * d + q) * a.B + c] = a.A[(size_t)k * kCloLen(d) + u];
  }
  if (a.gsave && threadIdx.x == 0) {     // several closures may meet in one state: one thread, the order they were added in
    for (int k = 0; k < a.count; k++) {
      const double *rec = a.A + (size_t)k * kCloLen(d);
      for (int side = 0; side < 2; side++) {
        const int s = side ? a.second[k] : a.first[k];
        for (int c = 0; c < d; c++) {
          double acc = 0.0;
          for (int q = 0; q < d; q++) acc += rec[side * d * d + q * d + c] * rec[2 * d * d + q];
          a.gsave[(size_t)s * a.B + c] += acc;
        }
      }
    }
  }
}

// Y = (I + U Z)^-1 ([r | 0] - U X): one wave.  W = U [X | Z] from the solution columns of the closures' states, Cholesky of the
// symmetrised I + U Z in LDS, one lane per right-hand side for the two substitutions.
template <int d> __global__ void __launch_bounds__(64) k_clo_solve(CloArgs a) {
  constexpr int NM = kMaxRhs - 1;
  __shared__ double W[NM][kMaxRhs + 1];
  __shared__ double C[NM][NM + 1];
  const int lane = threadIdx.x, nc = a.count * d, R = a.R;
  for (int idx = lane; idx < nc * R; idx += 64) {
    const int p = idx / R, c = idx - p * R;
    W[p][c] = clo_row_dot<d>(a.A, a.first, a.second, a.x, R, a.B, p, c);
  }
  wave_lds_sync();
  for (int idx = lane; idx < nc * nc; idx += 64) {
    const int p = idx / nc, p2 = idx - p * nc;
    C[p][p2] = (p == p2 ? 1.0 : 0.0) + 0.5 * (W[p][a.col0 + p2] + W[p2][a.col0 + p]);   // (clo_sym_entry)
  }
  wave_lds_sync();
  for (int j = 0; j < nc; j++) {      // right-looking Cholesky, lower triangle
    double dd = C[j][j];
    if (!(dd > 0.0)) { if (lane == 0) *a.flag = 1; dd = 1.0; }
    const double l = sqrt(dd), linv = 1.0 / l;
    wave_lds_sync();
    for (int i = j + lane; i < nc; i += 64) C[i][j] = (i == j) ? l : C[i][j] * linv;
    wave_lds_sync();
    const int m = nc - j - 1;
    for (int idx = lane; idx < m * m; idx += 64) {
      const int i = j + 1 + idx / m, k = j + 1 + idx % m;
      if (k <= i) C[i][k] -= C[i][j] * C[k][j];
    }
    wave_lds_sync();
  }
  if (lane < a.ncols) {               // lane c: column c of [r | 0] - U X through L y = b, L^T z = y
    const int c = lane;
    double y[NM];
    for (int p = 0; p < nc; p++) {
      const int k = p / d, q = p - k * d;
      double v = (c == 0 ? a.A[(size_t)k * kCloLen(d) + 2 * d * d + q] : 0.0) - W[p][c];
      for (int m = 0; m < p; m++) v -= C[p][m] * y[m];
      y[p] = v / C[p][p];
    }
    for (int p = nc - 1; p >= 0; p--) {
      double v = y[p];
      for (int m = p + 1; m < nc; m++) v -= C[m][p] * y[m];
      y[p] = v / C[p][p];
    }
    for (int p = 0; p < nc; p++) a.Y[(size_t)p * a.ncols + c] = y[p];
  }
}

// X <- X + Z Y on the update column and the landmark columns of every state
template <int d> __global__ void __launch_bounds__(256) k_clo_correct(CloArgs a) {
  const int nc = a.count * d;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = tid / a.B, k = tid - s * a.B;
  if (s >= a.N) return;
  double *xs = a.x + (size_t)s * a.R * a.B;
  double z[kMaxRhs - 1];
  for (int q = 0; q < nc; q++) z[q] = xs[(size_t)(a.col0 + q) * a.B + k];
  for (int c = 0; c < a.ncols; c++) {
    double v = xs[(size_t)c * a.B + k];
    for (int q = 0; q < nc; q++) v += z[q] * a.Y[(size_t)q * a.ncols + c];
    xs[(size_t)c * a.B + k] = v;
  }
}

// ---- closures in column passes (gpslam_hip_set_closure_passes): more closures than one border holds.  The nc = K d columns of U^T
// go through the chain solver a slice of w closures at a time (P = ceil(K / w) passes of the same factorisation, each at the same
// lambda), and only W = U [X | Z] -- Z at the closures' own two states -- is kept of them (nc x (ncols + nc), global memory).  Then
//   Y = (I + U Z)^-1 ([r | 0] - U X)   (k_clo_solve_wide, one workgroup),   X_full = X + H0^-1 (U^T Y):
// one more pass with U^T Y in place of [g | B] and the closure columns empty, added to the X saved from pass 0.
struct CloPass {
  int k0, k1;             // the closures of this pass's slice
  int lead;               // pass 0: the ncols leading columns U X are gathered as well
  double *W;              // nc x ldw
  int ldw;                // ncols + nc
  double *X;              // N x ncols x B: columns 0 .. ncols - 1 of pass 0's solution
};
constexpr int kCloWideMax = 120;    // rows of the wide system (closures * d)
constexpr int kCloWidePanel = 8;    // panel width of its Cholesky factorisation
// the dynamic LDS of the wide solve: the matrix (rows padded by one) and ncols right-hand sides
constexpr size_t clo_wide_lds(int nc, int ncols) { return ((size_t)nc * (nc + 1) + (size_t)nc * ncols) * sizeof(double); }
constexpr size_t kCloWideLds = clo_wide_lds(kCloWideMax, kMaxRhs);

// X <- columns 0 .. ncols - 1 of the level-0 solution (they lead every state's R x B record)
template <int d> __global__ void __launch_bounds__(256) k_clo_save(CloArgs a, CloPass p) {
  const int per = a.ncols * a.B;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)a.N * per) return;
  const size_t s = i / per;
  p.X[i] = a.x[s * a.R * a.B + (i - s * per)];
}

// W[:, slice] = U Z_slice (and W[:, 0 .. ncols - 1] = U X on pass 0): one thread per entry
template <int d> __global__ void __launch_bounds__(256) k_clo_gather(CloArgs a, CloPass p) {
  const int nc = a.count * d, R = a.R;
  const int nlead = p.lead ? a.ncols : 0, wid = nlead + (p.k1 - p.k0) * d;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nc * wid) return;
  const int row = idx / wid, cc = idx - row * wid;
  const int xc = cc < nlead ? cc : a.col0 + (cc - nlead);             // column of the solution
  const int wc = cc < nlead ? cc : a.ncols + p.k0 * d + (cc - nlead);   // column of W
  p.W[(size_t)row * p.ldw + wc] = clo_row_dot<d>(a.A, a.first, a.second, a.x, R, a.B, row, xc);
}

// Y = (I + 1/2 (U Z + (U Z)^T))^-1 ([r | 0] - U X), nc <= kCloWideMax: one workgroup, the matrix and the right-hand sides in dynamic
// LDS (nc (nc + 1) + nc ncols doubles).  Right-looking Cholesky in panels of kCloWidePanel columns, then the two substitutions, every
// entry owned by one thread between two barriers: the same sums in the same order on every run.
template <int d> __global__ void __launch_bounds__(256) k_clo_solve_wide(CloArgs a, CloPass p) {
  extern __shared__ double clo_lds[];
  const int tid = threadIdx.x, nc = a.count * d, ls = nc + 1, nr = a.ncols;
  double *S = clo_lds, *Rh = clo_lds + (size_t)nc * ls;
  for (int idx = tid; idx < nc * nc; idx += 256) {
    const int i = idx / nc, j = idx - i * nc;
    S[i * ls + j] = clo_sym_entry(i == j, p.W[(size_t)i * p.ldw + nr + j], p.W[(size_t)j * p.ldw + nr + i]);
  }
  for (int idx = tid; idx < nc * nr; idx += 256) {
    const int i = idx / nr, c = idx - i * nr;
    const int k = i / d, q = i - k * d;
    Rh[idx] = (c == 0 ? a.A[(size_t)k * kCloLen(d) + 2 * d * d + q] : 0.0) - p.W[(size_t)i * p.ldw + c];   // (as k_clo_solve's)
  }
  __syncthreads();
  for (int j0 = 0; j0 < nc; j0 += kCloWidePanel) {
    const int j1 = min(j0 + kCloWidePanel, nc);
    for (int j = j0; j < j1; j++) {     // the panel: column j, then its update of the panel's columns to the right
      double dd = S[j * ls + j];
      if (!(dd > 0.0)) { if (tid == 0) *a.flag = 1; dd = 1.0; }
      const double l = sqrt(dd), linv = 1.0 / l;
      __syncthreads();
      for (int i = j + tid; i < nc; i += 256) S[i * ls + j] = (i == j) ? l : S[i * ls + j] * linv;
      __syncthreads();
      const int pc = j1 - j - 1, pr = nc - j - 1;
      for (int idx = tid; idx < pr * pc; idx += 256) {
        const int i = j + 1 + idx / pc, k = j + 1 + idx % pc;
        if (k <= i) S[i * ls + k] -= S[i * ls + j] * S[k * ls + j];
      }
      __syncthreads();
    }
    const int m = nc - j1, jb = j1 - j0;   // the trailing matrix: rank-jb update, lower triangle
    for (int idx = tid; idx < m * m; idx += 256) {
      const int i = j1 + idx / m, k = j1 + idx % m;
      if (k <= i) {
        double acc = S[i * ls + k];
        for (int t = 0; t < jb; t++) acc -= S[i * ls + j0 + t] * S[k * ls + j0 + t];
        S[i * ls + k] = acc;
      }
    }
    __syncthreads();
  }
  for (int j = 0; j < nc; j++) {          // L y = b
    if (tid < nr) Rh[j * nr + tid] /= S[j * ls + j];
    __syncthreads();
    for (int idx = tid; idx < (nc - j - 1) * nr; idx += 256) {
      const int i = j + 1 + idx / nr, c = idx % nr;
      Rh[i * nr + c] -= S[i * ls + j] * Rh[j * nr + c];
    }
    __syncthreads();
  }
  for (int j = nc - 1; j >= 0; j--) {     // L^T z = y
    if (tid < nr) Rh[j * nr + tid] /= S[j * ls + j];
    __syncthreads();
    for (int idx = tid; idx < j * nr; idx += 256) {
      const int i = idx / nr, c = idx - i * nr;
      Rh[i * nr + c] -= S[j * ls + i] * Rh[j * nr + c];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < nc * nr; idx += 256) a.Y[idx] = Rh[idx];
}

// the final pass's right-hand sides: columns 0 .. ncols - 1 of every record emptied ...
template <int d> __global__ void __launch_bounds__(256) k_clo_clear_lead(CloArgs a) {
  const int per = a.ncols * a.B;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)a.N * per) return;
  const size_t s = i / per;
  a.blk[s * a.BS + 2 * a.B * a.B + (i - s * per)] = 0.0;
}
// ... and U^T Y added at the closures' states: one workgroup, a thread owns one (column, pose coordinate) through every closure, in
// the order they were added in
template <int d> __global__ void __launch_bounds__(256) k_clo_inject_y(CloArgs a) {
  for (int t = threadIdx.x; t < a.ncols * d; t += 256) {
    const int c = t / d, m = t - c * d;
    for (int k = 0; k < a.count; k++) {
      const double *rec = a.A + (size_t)k * kCloLen(d);
      for (int side = 0; side < 2; side++) {
        const int s = side ? a.second[k] : a.first[k];
        double acc = 0.0;
        for (int q = 0; q < d; q++) acc += rec[side * d * d + q * d + m] * a.Y[(size_t)(k * d + q) * a.ncols + c];
        a.blk[(size_t)s * a.BS + 2 * a.B * a.B + (size_t)c * a.B + m] += acc;
      }
    }
  }
}
// x[:, c] = X[:, c] + x[:, c], c < ncols
template <int d> __global__ void __launch_bounds__(256) k_clo_add(CloArgs a, CloPass p) {
  const int per = a.ncols * a.B;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)a.N * per) return;
  const size_t s = i / per;
  double *xs = a.x + s * a.R * a.B + (i - s * per);
  *xs = p.X[i] + *xs;
}

}  // namespace gps
