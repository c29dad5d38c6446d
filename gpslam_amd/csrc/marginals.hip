// marginals.hip -- gtsam::Marginals(graph, values) at the handle's current states: blocks of Sigma = H^-1, H = J^T J of the
// whole whitened graph (chain factors, measurements, landmark priors, loop closures; no damping), kept on the device.
//
//   (a) the level-0 records [D | O | G] of the current linearisation (the assembly gpslam_hip_normal_equations runs);
//   (b) selected inversion of the block-tridiagonal chain part A (k_mg_forward / k_mg_top / k_mg_backward): chunks of kMgChunk
//       states, the first state of a chunk its separator; the interiors are eliminated in order and fill the separator, the
//       separators form a block-tridiagonal system of the same kind, recursively, until one block is left; going back down,
//       each chunk turns the Sigma blocks of its two separators into Sigma_{j,j} and Sigma_{j,j+1} of its interiors;
//   (c) landmarks and closures as one low-rank term: the existing solver's right-hand sides give Y = [W | Z] (the landmark
//       columns corrected for the closures, H_xx^-1 B, and the closure columns A^-1 J_c^T), its landmark reduction the Schur
//       complement S = H_LL - B^T H_xx^-1 B; then Sigma_xx = A^-1 + Y K Y^T with K = blkdiag(S^-1, -(I + J_c Z)^-1),
//       Sigma_LL = S^-1, Sigma_xL = -W S^-1 (k_mg_core, k_mg_finish); on a handle whose closures go in column passes (clo.P > 1,
//       gpslam_hip_marginals_keep_closure_columns) Z is kept slice by slice and its term has kernels of its own (marginals_clo.hip);
//   (d) batched posterior covariances of GP-interpolated poses (k_mg_interp behind k_interp_query's H1..H4);
//   (e) a handle on the segmented landmark path (gpslam_hip_marginals_on_segments) takes none of (b), (c): marginals_fs.hip inverts
//       through the nested dissection and leaves Sigma_{i,i}, Sigma_{i,i+1} where (d) and get_marginals read them;
//   (f) Sigma_{a,b} of any two states and the closure gate over it walk what (b), (c) leave (marginals_pairs.hip), from a copy of Y
//       taken behind k_mg_finish when gpslam_hip_marginals_keep_pair_terms asked for it.
// fp64 only; no atomics, every sum in a fixed order: two calls give bit-identical blocks.
// What the call leaves is h->mg (marginals.hpp: struct Marginals, the levels' layout MgLevels, the shapes of Z and G); this file has the
// getters' guard marginals_getter_check and the pivot epilogue marginals_finish_flag that marginals_fs.hip ends with as well; the
// device helpers shared with the other three units (mg_set, mg_pads) are marginals_dev.hpp's.
#include "marginals_dev.hpp"

namespace impl64 {
#include "api_decl.inc"
}
namespace impl32 {
#include "api_decl.inc"
}

namespace {

constexpr int kMgMaxCols = kMaxRhs - 1;   // landmark coordinates + closure rows (<= 27)

template <int B> __device__ inline void mg_store(double *g, const double *l) {
  for (int e = threadIdx.x; e < B * B; e += 64) g[e] = l[e];
}

// In-place Gauss-Jordan inverse of an SPD matrix without pivoting: the pivots are the leading Schur complements, all positive
// exactly when the matrix is positive definite (a non-positive one raises the flag)
template <int B> __device__ inline void mg_inverse(double *M, int *flag) {
  for (int k = 0; k < B; k++) {
    double piv = M[k * B + k];
    if (!(piv > 0.0)) { if (threadIdx.x == 0) *flag = 1; piv = 1.0; }
    const double pinv = 1.0 / piv;
    mg_set<B>(M, [&](int i, int j) {
      if (i == k) return j == k ? pinv : M[k * B + j] * pinv;
      if (j == k) return -M[i * B + k] * pinv;
      return M[i * B + j] - M[i * B + k] * M[k * B + j] * pinv;
    });
  }
}
// the same for an n x n matrix (n <= kMgMaxCols, row stride ld)
__device__ inline void mg_inverse_n(double *M, int n, int ld, int *flag) {
  constexpr int NE = (kMgMaxCols * kMgMaxCols + 63) / 64;
  for (int k = 0; k < n; k++) {
    double piv = M[k * ld + k];
    if (!(piv > 0.0)) { if (threadIdx.x == 0) *flag = 1; piv = 1.0; }
    const double pinv = 1.0 / piv;
    double v[NE];
#pragma unroll
    for (int t = 0; t < NE; t++) {
      const int e = threadIdx.x + 64 * t;
      if (e < n * n) {
        const int i = e / n, j = e - i * n;
        if (i == k) v[t] = (j == k) ? pinv : M[k * ld + j] * pinv;
        else if (j == k) v[t] = -M[i * ld + k] * pinv;
        else v[t] = M[i * ld + j] - M[i * ld + k] * M[k * ld + j] * pinv;
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NE; t++) {
      const int e = threadIdx.x + 64 * t;
      if (e < n * n) M[(e / n) * ld + e % n] = v[t];
    }
    __syncthreads();
  }
}

// One level of the selected inversion.  D, O: diagonal blocks and O_i = A_{i+1,i} (row-major, the records' convention) with a
// record stride; add: blocks subtracted from D (fill a left chunk left in its right separator) or null.
struct MgLevel {
  const double *D, *O, *add;
  int stride, n;
  double *fac;                  // n x 3 B^2: [P_j^-1 | U_j | V_j] of each interior state j
  double *upD, *upO, *upAdd;    // the separators' system: ceil(n / kMgChunk) blocks, upAdd[0] zero
  double *Sd, *Sn;              // n x B^2 each: Sigma_{i,i}, Sigma_{i,i+1} (rows: state i)
  const double *upSd, *upSn;    // the same of the level above
  int *flag;
};

// Eliminate the interiors of one chunk (one wave per chunk):
//   P_{s+1} = D_{s+1},  F_{s+1} = E_s^T,  U_j = P_j^-1 E_j,  V_j = P_j^-1 F_j,  D_s -= F_j^T V_j,
//   P_{j+1} = D_{j+1} - E_j^T U_j,  F_{j+1} = -E_j^T V_j;  the last interior: D_r -= E_j^T U_j (-> upAdd), A'_{r,s} = -E_j^T V_j
template <int B> __global__ void __launch_bounds__(64) k_mg_forward(MgLevel a) {
  constexpr int BB = B * B;
  __shared__ double Ds[BB], P[BB], F[BB], U[BB], V[BB], E[BB];
  const int k = blockIdx.x, s = k * kMgChunk, e = min(s + kMgChunk, a.n);
  const bool right = e < a.n;
  auto Dg = [&](int i, int idx) { return a.D[(size_t)i * a.stride + idx] - (a.add ? a.add[(size_t)i * BB + idx] : 0.0); };
  auto Og = [&](int i) { return a.O + (size_t)i * a.stride; };
  mg_set<B>(Ds, [&](int r, int c) { return Dg(s, r * B + c); });
  if (e == s + 1) {                 // a chunk of one state: its coupling to the right separator is the chain's own
    mg_set<B>(F, [&](int r, int c) { return right ? Og(s)[r * B + c] : 0.0; });
    mg_store<B>(a.upD + (size_t)k * BB, Ds);
    mg_store<B>(a.upO + (size_t)k * BB, F);
    return;
  }
  mg_set<B>(P, [&](int r, int c) { return Dg(s + 1, r * B + c); });
  mg_set<B>(F, [&](int r, int c) { return Og(s)[r * B + c]; });
  for (int j = s + 1; j < e; j++) {
    mg_inverse<B>(P, a.flag);
    const bool hasE = j + 1 < a.n;
    mg_set<B>(E, [&](int r, int c) { return hasE ? Og(j)[c * B + r] : 0.0; });   // A_{j,j+1}
    mg_set<B>(U, [&](int r, int c) { double acc = 0.0; for (int q = 0; q < B; q++) acc += P[r * B + q] * E[q * B + c]; return acc; });
    mg_set<B>(V, [&](int r, int c) { double acc = 0.0; for (int q = 0; q < B; q++) acc += P[r * B + q] * F[q * B + c]; return acc; });
    double *f = a.fac + (size_t)j * 3 * BB;
    mg_store<B>(f, P);
    mg_store<B>(f + BB, U);
    mg_store<B>(f + 2 * BB, V);
    mg_set<B>(Ds, [&](int r, int c) { double acc = Ds[r * B + c]; for (int q = 0; q < B; q++) acc -= F[q * B + r] * V[q * B + c]; return acc; });
    if (j + 1 < e) {
      mg_set<B>(P, [&](int r, int c) { double acc = Dg(j + 1, r * B + c); for (int q = 0; q < B; q++) acc -= E[q * B + r] * U[q * B + c]; return acc; });
      mg_set<B>(F, [&](int r, int c) { double acc = 0.0; for (int q = 0; q < B; q++) acc -= E[q * B + r] * V[q * B + c]; return acc; });
    } else {
      mg_set<B>(P, [&](int r, int c) { double acc = 0.0; for (int q = 0; q < B; q++) acc += E[q * B + r] * U[q * B + c]; return acc; });
      mg_set<B>(F, [&](int r, int c) { double acc = 0.0; for (int q = 0; q < B; q++) acc -= E[q * B + r] * V[q * B + c]; return acc; });
      if (right) mg_store<B>(a.upAdd + (size_t)(k + 1) * BB, P);
      mg_store<B>(a.upO + (size_t)k * BB, F);     // (zero without a right separator: E = 0)
    }
  }
  mg_store<B>(a.upD + (size_t)k * BB, Ds);
}

// the top of the recursion: one block, Sigma = (D - add)^-1
template <int B> __global__ void __launch_bounds__(64) k_mg_top(MgLevel a) {
  constexpr int BB = B * B;
  __shared__ double M[BB];
  mg_set<B>(M, [&](int r, int c) { return a.D[r * B + c] - (a.add ? a.add[r * B + c] : 0.0); });
  mg_inverse<B>(M, a.flag);
  mg_store<B>(a.Sd, M);
  for (int e = threadIdx.x; e < BB; e += 64) a.Sn[e] = 0.0;
}

// Back down one level (one wave per chunk), from Sigma_{s,s}, Sigma_{r,r}, Sigma_{s,r} of the chunk's separators; n = j + 1:
//   Sigma_{j,s} = -U_j Sigma_{n,s} - V_j Sigma_{s,s},  Sigma_{j,n} = -U_j Sigma_{n,n} - V_j Sigma_{n,s}^T,
//   Sigma_{j,j} = P_j^-1 - U_j Sigma_{j,n}^T - V_j Sigma_{j,s}^T
template <int B> __global__ void __launch_bounds__(64) k_mg_backward(MgLevel a) {
  constexpr int BB = B * B;
  __shared__ double Sss[BB], Sns[BB], Snn[BB], Sjs[BB], Sjn[BB], Pi[BB], U[BB], V[BB];
  const int k = blockIdx.x, s = k * kMgChunk, e = min(s + kMgChunk, a.n);
  const bool right = e < a.n;
  const double *up_ss = a.upSd + (size_t)k * BB, *up_sr = a.upSn + (size_t)k * BB;
  mg_set<B>(Sss, [&](int r, int c) { return up_ss[r * B + c]; });
  mg_store<B>(a.Sd + (size_t)s * BB, Sss);
  if (e == s + 1) {
    for (int t = threadIdx.x; t < BB; t += 64) a.Sn[(size_t)s * BB + t] = right ? up_sr[t] : 0.0;
    return;
  }
  mg_set<B>(Snn, [&](int r, int c) { return right ? a.upSd[(size_t)(k + 1) * BB + r * B + c] : 0.0; });
  mg_set<B>(Sns, [&](int r, int c) { return right ? up_sr[c * B + r] : 0.0; });
  for (int j = e - 1; j > s; j--) {
    const double *f = a.fac + (size_t)j * 3 * BB;
    mg_set<B>(Pi, [&](int r, int c) { return f[r * B + c]; });
    mg_set<B>(U, [&](int r, int c) { return f[BB + r * B + c]; });
    mg_set<B>(V, [&](int r, int c) { return f[2 * BB + r * B + c]; });
    mg_set<B>(Sjs, [&](int r, int c) {
      double acc = 0.0;
      for (int q = 0; q < B; q++) acc -= U[r * B + q] * Sns[q * B + c];
      for (int q = 0; q < B; q++) acc -= V[r * B + q] * Sss[q * B + c];
      return acc;
    });
    mg_set<B>(Sjn, [&](int r, int c) {
      double acc = 0.0;
      for (int q = 0; q < B; q++) acc -= U[r * B + q] * Snn[q * B + c];
      for (int q = 0; q < B; q++) acc -= V[r * B + q] * Sns[c * B + q];
      return acc;
    });
    mg_set<B>(Snn, [&](int r, int c) {     // Sigma_{j,j}: the next step's Sigma_{n,n}
      double acc = Pi[r * B + c];
      for (int q = 0; q < B; q++) acc -= U[r * B + q] * Sjn[c * B + q];
      for (int q = 0; q < B; q++) acc -= V[r * B + q] * Sjs[c * B + q];
      return acc;
    });
    mg_store<B>(a.Sd + (size_t)j * BB, Snn);
    mg_store<B>(a.Sn + (size_t)j * BB, Sjn);
    mg_set<B>(Sns, [&](int r, int c) { return Sjs[r * B + c]; });
  }
  for (int t = threadIdx.x; t < BB; t += 64) a.Sn[(size_t)s * BB + t] = Sns[(t % B) * B + t / B];   // Sigma_{s,s+1} = Sigma_{s+1,s}^T
}

// K = blkdiag(S^-1, -(I + J_c Z)^-1), one wave.  S: the landmark reduction's Schur complement (upper part, as k_lm_solve reads
// it); J_c Z from the closures' whitened Jacobians and the closure columns of the solution at their two states (clo_row_dot's sums, spelt out: with the helper the code of k_mg_core<2> changes).
struct MgCore {
  const double *S;              // nl x R, columns 1 .. nl
  const double *cloA;           // closure records [A_i | A_j | r]
  const int *first, *second;
  const double *x;              // level-0 solutions N x R x B
  int nl, nclo, R, B;
  double *K;                    // m x m, m = nl + nclo d
  double *Slm;                  // nl x nl
  int *flag;
};
template <int d> __global__ void __launch_bounds__(64) k_mg_core(MgCore a) {
  __shared__ double Sm[kMgMaxCols * kMgMaxCols], Mm[kMgMaxCols * kMgMaxCols];
  const int lane = threadIdx.x, nl = a.nl, nc = a.nclo * d, m = nl + nc, R = a.R;
  for (int idx = lane; idx < nl * nl; idx += 64) {
    const int i = idx / nl, j = idx - i * nl;
    Sm[i * kMgMaxCols + j] = a.S[(size_t)min(i, j) * R + 1 + max(i, j)];
  }
  for (int idx = lane; idx < nc * nc; idx += 64) {   // (J_c Z)[p][c] + (J_c Z)[c][p], halved: symmetric like k_clo_solve's
    const int p = idx / nc, c = idx - p * nc;
    double w[2];
    for (int side = 0; side < 2; side++) {
      const int pp = side ? c : p, cc = side ? p : c;
      const int kk = pp / d, q = pp - kk * d;
      const double *rec = a.cloA + (size_t)kk * kCloLen(d);
      const double *xi = a.x + ((size_t)a.first[kk] * R + 1 + nl + cc) * a.B, *xj = a.x + ((size_t)a.second[kk] * R + 1 + nl + cc) * a.B;
      double acc = 0.0;
      for (int u = 0; u < d; u++) acc += rec[q * d + u] * xi[u];
      for (int u = 0; u < d; u++) acc += rec[d * d + q * d + u] * xj[u];
      w[side] = acc;
    }
    Mm[p * kMgMaxCols + c] = clo_sym_entry(p == c, w[0], w[1]);
  }
  __syncthreads();
  mg_inverse_n(Sm, nl, kMgMaxCols, a.flag);
  mg_inverse_n(Mm, nc, kMgMaxCols, a.flag);
  for (int idx = lane; idx < m * m; idx += 64) {
    const int i = idx / m, j = idx - i * m;
    double v = 0.0;
    if (i < nl && j < nl) v = Sm[i * kMgMaxCols + j];
    else if (i >= nl && j >= nl) v = -Mm[(i - nl) * kMgMaxCols + (j - nl)];
    a.K[idx] = v;
  }
  for (int idx = lane; idx < nl * nl; idx += 64) a.Slm[idx] = Sm[(idx / nl) * kMgMaxCols + idx % nl];
}

// Per state i and row r: Sigma_{i,i} += Y_i K Y_i^T, Sigma_{i,i+1} += Y_i K Y_{i+1}^T, Sigma_{i,L} = -(Y_i K)[:, :nl]; then the
// coordinates that are no variable (ROT3_BIAS: the three pad components of the velocity slot) report zero rows and columns
struct MgFinish {
  double *Sd, *Sn, *Sxl;
  const double *x, *K;
  int N, R, m, nl;
  int pad0, npad;               // padding coordinates pad0 .. pad0 + npad - 1 of each state
};
template <int B> __global__ void __launch_bounds__(256) k_mg_finish(MgFinish a) {
  constexpr int BB = B * B;
  __shared__ double K[kMgMaxCols * kMgMaxCols];
  for (int idx = threadIdx.x; idx < a.m * a.m; idx += 256) K[idx] = a.K[idx];
  __syncthreads();
  const int tid = blockIdx.x * 256 + threadIdx.x;
  const int i = tid / B, r = tid - i * B;
  if (i >= a.N) return;
  const int R = a.R, m = a.m;
  const bool next = i + 1 < a.N;
  double *sd = a.Sd + (size_t)i * BB + r * B, *sn = a.Sn + (size_t)i * BB + r * B;
  if (m > 0) {
    const double *xi = a.x + (size_t)i * R * B, *xn = a.x + (size_t)(i + 1) * R * B;
    double T[kMgMaxCols];
#pragma unroll
    for (int c = 0; c < kMgMaxCols; c++) {
      double acc = 0.0;
      if (c < m)
        for (int q = 0; q < m; q++) acc += xi[(size_t)(1 + q) * B + r] * K[q * m + c];
      T[c] = acc;
    }
    for (int cc = 0; cc < B; cc++) {
      double acc = 0.0, acc2 = 0.0;
#pragma unroll
      for (int c = 0; c < kMgMaxCols; c++)
        if (c < m) {
          acc += T[c] * xi[(size_t)(1 + c) * B + cc];
          if (next) acc2 += T[c] * xn[(size_t)(1 + c) * B + cc];
        }
      sd[cc] += acc;
      if (next) sn[cc] += acc2;
    }
#pragma unroll
    for (int c = 0; c < kMgMaxCols; c++)
      if (c < a.nl) a.Sxl[((size_t)i * B + r) * a.nl + c] = -T[c];
  }
  if (a.npad > 0) {
    const bool rp = r >= a.pad0 && r < a.pad0 + a.npad;
    for (int cc = 0; cc < B; cc++)
      if (rp || (cc >= a.pad0 && cc < a.pad0 + a.npad)) { sd[cc] = 0.0; sn[cc] = 0.0; }
    if (rp)
      for (int c = 0; c < a.nl; c++) a.Sxl[((size_t)i * B + r) * a.nl + c] = 0.0;
  }
}

// P(tau) = H_J Sigma_J H_J^T + g c Q_c, thread per query; H_J = [H1 H2 H3 H4] (d x 2B) from k_interp_query,
// Sigma_J = [[S_i, Sn_i], [Sn_i^T, S_{i+1}]], c = tau^3 (dt - tau)^3 / (3 dt^3) (host), Q_c on the first nq coordinates
struct MgInterp {
  const double *H, *cg, *Qc;    // count x 4 d^2, count (g c), d x d
  const int *left;
  const double *Sd, *Sn;
  int count, nq;
  double *out;                  // count x d x d
};
template <int B> __global__ void __launch_bounds__(128) k_mg_interp(MgInterp a) {
  constexpr int d = B / 2, BB = B * B;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.count) return;
  const int i = a.left[q];
  const double *H = a.H + (size_t)q * 4 * d * d;
  const double *S0 = a.Sd + (size_t)i * BB, *S1 = a.Sd + (size_t)(i + 1) * BB, *Sx = a.Sn + (size_t)i * BB;
  auto hj = [&](int r, int col) { return H[((col / d) * d + r) * d + col % d]; };
  auto sj = [&](int u, int v) {
    if (u < B) return v < B ? S0[u * B + v] : Sx[u * B + v - B];
    return v < B ? Sx[v * B + u - B] : S1[(u - B) * B + v - B];
  };
  const double gc = a.cg[q];
  for (int r = 0; r < d; r++) {
    double t[2 * B];
#pragma unroll
    for (int v = 0; v < 2 * B; v++) {
      double acc = 0.0;
      for (int u = 0; u < 2 * B; u++) acc += hj(r, u) * sj(u, v);
      t[v] = acc;
    }
    for (int c = 0; c < d; c++) {
      double acc = 0.0;
#pragma unroll
      for (int v = 0; v < 2 * B; v++) acc += t[v] * hj(c, v);
      if (r < a.nq && c < a.nq) acc += gc * a.Qc[r * d + c];
      a.out[((size_t)q * d + r) * d + c] = acc;
    }
  }
}

int mg_refuse(gpslam_hip_handle *h) {
  if (h->cfg.precision == GPSLAM_FP32) return fail(h, GPSLAM_E_UNSUPPORTED, "marginals: fp32 handles are not supported (fp64 only)");
  if (sharded(h)) return fail(h, GPSLAM_E_UNSUPPORTED, "marginals: sharded handles are not supported");
  if (h->fs.active && h->fs.split) return fail(h, GPSLAM_E_UNSUPPORTED, "marginals: split pieces are not supported");
  if (h->fs.active && !h->mg.on_segments) return fail(h, GPSLAM_E_UNSUPPORTED, "marginals: the segmented landmark path is not supported");
  if (h->clo.P > 1 && !h->mg.keep_z)
    return fail(h, GPSLAM_E_UNSUPPORTED, "marginals: loop closures in more than one column pass (set_closure_passes) are not supported: Z = H0^-1 U^T is not kept at every state (unless gpslam_hip_marginals_keep_closure_columns asks for it)");
  return 0;
}

int mg_stale(gpslam_hip_handle *h) {
  if (!h->mg.ok) return fail(h, GPSLAM_E_INVALID, "marginals are stale: call gpslam_hip_marginals() after the last change of states, landmarks, factors or Qc");
  return 0;
}

}  // namespace

int marginals_getter_check(gpslam_hip_handle *h) {
  const int rc = mg_refuse(h);
  return rc ? rc : mg_stale(h);
}

int marginals_finish_flag(gpslam_hip_handle *h) {
  int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (flag) return fail(h, GPSLAM_E_NOT_SPD, "marginals: non-positive pivot (indeterminate system: is the graph anchored?)");
  h->mg.ok = true;
  return 0;
}

extern "C" {

int gpslam_hip_marginals_keep_closure_columns(gpslam_hip_handle *h, int32_t enable) {
  if (!h) return GPSLAM_E_INVALID;
  h->mg.invalidate();
  h->mg.keep_z = enable != 0;
  if (!h->mg.keep_z) {   // freed now: Z is the marginals' largest buffer (N b x nc) and nothing reads it without the opt-in
    h->mg.Z.release();
    h->mg.Minv.release();
  }
  return 0;
}

int gpslam_hip_marginals_on_segments(gpslam_hip_handle *h, int32_t enable) {
  if (!h) return GPSLAM_E_INVALID;
  h->mg.invalidate();
  h->mg.on_segments = enable != 0;
  if (!h->mg.on_segments)   // freed now: G is N b x NCP, and nothing reads the three without the opt-in
    for (DevBuf *b : {&h->mg.fsD, &h->mg.fsP, &h->mg.G}) b->release();
  return 0;
}

int gpslam_hip_marginals(gpslam_hip_handle *h) {
  int rc = need_compiled(h);
  if (rc) return rc;
  if ((rc = mg_refuse(h))) return rc;
  (void)hipSetDevice(h->cfg.device);
  h->mg.invalidate();
  if (h->fs.active) return marginals_fs(h);
  const int N = h->N, B = h->b, BB = B * B, R = h->R, m = R - 1;
  const MgLevels lv(N, B);
  const int top = lv.top;
  h->mg.fit(N);   // (another N than the last call's: its buffers are freed first, not grown)
  HIPCHK(h->mg.fac.reserve((size_t)N * 3 * BB * sizeof(double)));
  HIPCHK(h->mg.S.reserve((size_t)N * BB * sizeof(double)));
  HIPCHK(h->mg.Sn.reserve((size_t)N * BB * sizeof(double)));
  HIPCHK(h->mg.up.reserve(std::max<size_t>(lv.total(), 1) * sizeof(double)));
  HIPCHK(h->mg.K.reserve((size_t)std::max(m * m, 1) * sizeof(double)));
  HIPCHK(h->mg.Slm.reserve((size_t)std::max(h->nl * h->nl, 1) * sizeof(double)));
  HIPCHK(h->mg.Sxl.reserve((size_t)std::max(N * B * h->nl, 1) * sizeof(double)));
  const bool passes = h->clo.P > 1;     // (mg_refuse: only with gpslam_hip_marginals_keep_closure_columns)
  const int ldz = mg_ldz(h->clo.nc);
  if (passes) {
    const size_t zbytes = mg_zrows(N, B) * ldz * sizeof(double);
    HIPCHK(h->mg.Z.reserve(zbytes));
    HIPCHK(h->mg.Minv.reserve((size_t)ldz * ldz * sizeof(double)));
    HIPCHK(hipMemsetAsync(h->mg.Z.p, 0, zbytes, h->stream));   // the padding rows and columns: k_mg_clo_finish reads them
  }
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  if ((rc = impl64::launch_factors(h, LaunchMode{}, 0, 0)) || (rc = impl64::launch_assemble(h, LaunchMode{}, false))) return rc;
  const double *blk = h->lv[0].blk.as<double>();
  const int BS = 2 * BB + B * R;
  auto level = [&](int l) {
    MgLevel a;
    double *up = h->mg.up.as<double>();
    if (l == 0) {
      a.D = blk; a.O = blk + BB; a.add = nullptr; a.stride = BS;
      a.fac = h->mg.fac.as<double>(); a.Sd = h->mg.S.as<double>(); a.Sn = h->mg.Sn.as<double>();
    } else {
      a.D = up + lv.D(l); a.O = up + lv.O(l); a.add = up + lv.add(l); a.stride = BB;
      a.fac = up + lv.fac(l); a.Sd = up + lv.Sd(l); a.Sn = up + lv.Sn(l);
    }
    a.n = lv.n[l];
    a.upD = a.upO = a.upAdd = a.Sd; a.upSd = a.upSn = a.Sd;   // (unused on the top level)
    if (l < top) {
      a.upD = up + lv.D(l + 1); a.upO = up + lv.O(l + 1); a.upAdd = up + lv.add(l + 1); a.upSd = up + lv.Sd(l + 1); a.upSn = up + lv.Sn(l + 1);
    }
    a.flag = h->flag.as<int>();
    return a;
  };
  // (b) selected inversion of the chain part: reads D / O of the records before the solver below factors them in place
  for (int l = 0; l < top; l++) {
    const MgLevel a = level(l);
    HIPCHK(hipMemsetAsync(a.upAdd, 0, (size_t)BB * sizeof(double), h->stream));
    dispatch_b(B, [&](auto tag) { k_mg_forward<decltype(tag)::value><<<dim3(lv.n[l + 1]), dim3(64), 0, h->stream>>>(a); });
  }
  dispatch_b(B, [&](auto tag) { k_mg_top<decltype(tag)::value><<<dim3(1), dim3(64), 0, h->stream>>>(level(top)); });
  for (int l = top - 1; l >= 0; l--) {
    const MgLevel a = level(l);
    dispatch_b(B, [&](auto tag) { k_mg_backward<decltype(tag)::value><<<dim3(lv.n[l + 1]), dim3(64), 0, h->stream>>>(a); });
  }
  HIPCHK(hipGetLastError());
  // (c) landmarks and closures: Y = [W | Z] and S from the solver's own right-hand sides, then K
  if (m > 0) {
    // closures in column passes: Z slice by slice into mg.Z, then - Z M^-1 Z^T on its own; what is left for k_mg_core and
    // k_mg_finish is the landmark term (W in the leading columns of the level-0 solution, K = S^-1: no closure reaches k_mg_core)
    LaunchMode border;
    border.keep_z = true; border.lm_reduce_only = true;
    if ((rc = impl64::launch_solve(h, border, 0.0))) return rc;
    if (passes && (rc = marginals_closure_term(h))) return rc;
    if (!passes || h->nl > 0) {
      MgCore c;
      c.S = h->lm_S.as<double>(); c.cloA = h->clo.A.as<double>(); c.first = h->clo.fac.d_idx.as<int>(); c.second = h->clo.d_second.as<int>();
      c.x = h->lv[0].x.as<double>(); c.nl = h->nl; c.nclo = passes ? 0 : h->clo.n; c.R = R; c.B = B;
      c.K = h->mg.K.as<double>(); c.Slm = h->mg.Slm.as<double>(); c.flag = h->flag.as<int>();
      dispatch_b(B, [&](auto tag) { k_mg_core<decltype(tag)::value / 2><<<dim3(1), dim3(64), 0, h->stream>>>(c); });
    }
  }
  const MgPads pads = mg_pads(h);
  const int mfin = passes ? h->nl : m;   // the columns k_mg_finish adds: [W | Z], or W alone behind k_mg_clo_finish
  if (mfin > 0 || pads.npad > 0) {
    MgFinish f;
    f.Sd = h->mg.S.as<double>(); f.Sn = h->mg.Sn.as<double>(); f.Sxl = h->mg.Sxl.as<double>();
    f.x = h->lv[0].x.as<double>(); f.K = h->mg.K.as<double>();
    f.N = N; f.R = R; f.m = mfin; f.nl = h->nl;
    f.pad0 = pads.pad0; f.npad = pads.npad;
    dispatch_b(B, [&](auto tag) { k_mg_finish<decltype(tag)::value><<<dim3(nblocks(N * B, 256)), dim3(256), 0, h->stream>>>(f); });
  }
  HIPCHK(hipGetLastError());
  if ((rc = marginals_pairs_keep(h))) return rc;   // (gpslam_hip_marginals_keep_pair_terms: Y before a later call rewrites it)
  return marginals_finish_flag(h);
}

int gpslam_hip_get_marginals(gpslam_hip_handle *h, int32_t first, int32_t count, double *S, double *S_next, double *S_lm,
                             double *S_x_lm) {
  if (!h) return GPSLAM_E_INVALID;
  int rc = mg_refuse(h);
  if (rc || (rc = mg_stale(h))) return rc;
  if (first < 0 || count < 0 || first + count > h->N) return fail(h, GPSLAM_E_INVALID, "get_marginals: state window out of range");
  if (h->fs.active && (S_lm || S_x_lm))
    return fail(h, GPSLAM_E_UNSUPPORTED, "get_marginals: S_lm / S_x_lm do not exist on the segmented landmark path (nl x nl, N b x nl); use "
                "gpslam_hip_get_landmark_marginals, gpslam_hip_get_state_landmark_marginals, gpslam_hip_get_landmark_pair_marginals");
  (void)hipSetDevice(h->cfg.device);
  const size_t BB = (size_t)h->b * h->b, nl = (size_t)h->nl;
  if (S && count) HIPCHK(hipMemcpyAsync(S, h->mg.S.as<double>() + first * BB, count * BB * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (S_next && count) HIPCHK(hipMemcpyAsync(S_next, h->mg.Sn.as<double>() + first * BB, count * BB * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (S_lm && nl) HIPCHK(hipMemcpyAsync(S_lm, h->mg.Slm.p, nl * nl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (S_x_lm && nl && count)
    HIPCHK(hipMemcpyAsync(S_x_lm, h->mg.Sxl.as<double>() + (size_t)first * h->b * nl, (size_t)count * h->b * nl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int gpslam_hip_get_landmark_marginals(gpslam_hip_handle *h, int32_t first, int32_t count, double *out) {
  if (!h || count < 0 || (count > 0 && !out)) return GPSLAM_E_INVALID;
  int rc = mg_refuse(h);
  if (rc || (rc = mg_stale(h))) return rc;
  if (first < 0 || first + count > h->L) return fail(h, GPSLAM_E_INVALID, "get_landmark_marginals: landmark window out of range");
  (void)hipSetDevice(h->cfg.device);
  std::vector<int32_t> idx(count);
  for (int t = 0; t < count; t++) idx[t] = first + t;
  return marginals_fs_gather(h, kMgGatherLmPair, count, idx.data(), idx.data(), out);
}

int gpslam_hip_get_state_landmark_marginals(gpslam_hip_handle *h, int32_t count, const int32_t *state, const int32_t *landmark, double *out) {
  if (!h || count < 0 || (count > 0 && (!state || !landmark || !out))) return GPSLAM_E_INVALID;
  int rc = mg_refuse(h);
  if (rc || (rc = mg_stale(h))) return rc;
  (void)hipSetDevice(h->cfg.device);
  return marginals_fs_gather(h, kMgGatherStateLm, count, state, landmark, out);
}

int gpslam_hip_get_landmark_pair_marginals(gpslam_hip_handle *h, int32_t count, const int32_t *a, const int32_t *b, double *out) {
  if (!h || count < 0 || (count > 0 && (!a || !b || !out))) return GPSLAM_E_INVALID;
  int rc = mg_refuse(h);
  if (rc || (rc = mg_stale(h))) return rc;
  (void)hipSetDevice(h->cfg.device);
  return marginals_fs_gather(h, kMgGatherLmPair, count, a, b, out);
}

int gpslam_hip_interpolate_covariances(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *dt,
                                       const double *tau, int32_t gp_term, double *out_cov) {
  if (!h || count < 0 || (count > 0 && (!left || !dt || !tau || !out_cov))) return GPSLAM_E_INVALID;
  int rc = mg_refuse(h);
  if (rc || (rc = mg_stale(h))) return rc;
  if (h->N < 2) return fail(h, GPSLAM_E_INVALID, "interpolation needs at least two states");
  for (int q = 0; q < count; q++) {
    if (left[q] < 0 || left[q] > h->N - 2) return fail(h, GPSLAM_E_INVALID, "query interval out of range");
    if (!(dt[q] > 0.0)) return fail(h, GPSLAM_E_INVALID, "delta_t must be positive");
  }
  if (count == 0) return 0;
  (void)hipSetDevice(h->cfg.device);
  const int d = h->d, pd = h->pd;
  std::vector<double> coef((size_t)count * 4), cg(count);
  for (int q = 0; q < count; q++) {
    interp_coef(dt[q], tau[q], &coef[4 * (size_t)q]);
    const double t = tau[q], s = dt[q] - tau[q];   // the position block of Q(tau) - Psi Phi(dt - tau) Q(tau), over Qc
    cg[q] = gp_term ? t * t * t * s * s * s / (3.0 * dt[q] * dt[q] * dt[q]) : 0.0;
  }
  std::vector<int> li(left, left + count);
  std::vector<double> qc(h->Qc, h->Qc + d * d);
  struct { DevBuf left, coef, cg, qc, pose, H, out; } sc;   // this call's own buffers
  if ((rc = upload(h, sc.left, li)) || (rc = upload(h, sc.coef, coef)) || (rc = upload(h, sc.cg, cg)) || (rc = upload(h, sc.qc, qc))) return rc;
  HIPCHK(sc.pose.reserve((size_t)count * pd * sizeof(double)));
  HIPCHK(sc.H.reserve((size_t)count * 4 * d * d * sizeof(double)));
  HIPCHK(sc.out.reserve((size_t)count * d * d * sizeof(double)));
  QueryArgs<double> a;
  a.pose = h->pose.as<double>(); a.vel = h->vel.as<double>(); a.stride = h->stride; a.count = count;
  a.left = sc.left.as<int>(); a.coef = sc.coef.as<double>(); a.out = sc.pose.as<double>(); a.out_H = sc.H.as<double>();
  a.vw = h->vw;
  dispatch_mf(h->mf, [&](auto tag) {
    k_interp_query<double, decltype(tag)::value, true><<<dim3(nblocks(count, 128)), dim3(128), 0, h->stream>>>(a);
  });
  MgInterp u;
  u.H = sc.H.as<double>(); u.cg = sc.cg.as<double>(); u.Qc = sc.qc.as<double>(); u.left = sc.left.as<int>();
  u.Sd = h->mg.S.as<double>(); u.Sn = h->mg.Sn.as<double>(); u.count = count;
  u.nq = h->mf == ROT3_BIAS ? 3 : d;   // (the bias is held over the interval, not interpolated)
  u.out = sc.out.as<double>();
  dispatch_b(h->b, [&](auto tag) { k_mg_interp<decltype(tag)::value><<<dim3(nblocks(count, 128)), dim3(128), 0, h->stream>>>(u); });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out_cov, sc.out.p, (size_t)count * d * d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"
