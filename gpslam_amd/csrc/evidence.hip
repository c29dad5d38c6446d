// evidence.hip -- log det H and the Laplace log-evidence of a handle (include/gpslam_hip_evidence.h):
//   log Z = -cost(x^) + sum_f log|det R_f| - 1/2 log det H - ((m - n) / 2) log 2 pi,   H = J^T J as gpslam_hip_marginals defines it.
// log det H = log det A + log det(I + U Z) + log det S:
//   (a) the level-0 records [D | O | G] of the current linearisation (launch_factors, launch_assemble);
//   (b) log det A of the block-tridiagonal chain part: the chunked elimination of marginals.hip (b), its forward half only
//       (k_ev_forward / k_ev_top).  Chunks of kMgChunk states, the first of a chunk its separator; the interiors are eliminated in
//       order, fill the separator and leave ONE number, the sum of the logarithms of their pivots; the separators form a system of
//       the same kind, recursively, until one block is left.  Nothing is stored per interior state: a pivot block is factorised by
//       Cholesky with [E | F] riding along (one forward substitution gives L^-1 E and L^-1 F, and every Schur update is a product
//       of those two), so there is no inverse, no [P^-1 | U | V], and no backward sweep;
//   (c) the solver's own right-hand sides at lambda = 0 (launch_solve, lm_reduce_only) give Z = A^-1 U^T at the closures' states -- in column
//       passes W = U [X | Z] in clo.W -- and the landmarks' Schur complement S in lm_S; k_ev_core takes the two log-determinants by
//       Cholesky in LDS, I + U Z symmetrised as k_mg_core / k_clo_solve_wide do (clo_sym_entry);
//   (d) k_ev_reduce adds the per-chunk partial sums of every level in a fixed order and writes the three parts and the pivot flag
//       where ONE copy reads them.
// fp64 only; no atomics, every sum in a fixed order, every grid a function of N alone: two calls give the same bits.
// The host arithmetic (the noise models' normaliser, the combination) is at the end: gpslam_hip_gp_log_normaliser and
// gpslam_hip_evidence_combine are all of it, and the handle entry points call them.
#include "api_common.hpp"
#include "../../include/gpslam_hip_evidence.h"

#include <atomic>
#include <cmath>

namespace impl64 {
#include "api_decl.inc"
}

namespace {

constexpr int kEvCoreThreads = 256;
constexpr int kEvReduceThreads = 256;
// A pivot of the chain's elimination counts as non-positive when it is below 2^-36 (1.5e-11) of the diagonal entry the same
// coordinate of the same state has in H: what is left of that entry is rounding (cancellation ate 36 of its 53 bits; a Jacobi-scaled
// condition number of 1e9, the most any test admits, leaves pivots at 1e-9 of it).  The plain test piv > 0 does not see an
// indeterminate system here: the products E^^T E^, F^^T F^ are symmetric to the bit and the block they cancel against comes out as
// a tiny positive definite residue as often as not -- the unanchored chain of the tests did
constexpr double kEvPivotFloor = 0x1p-36;

// One level of the elimination.  D, O: diagonal blocks and O_i = A_{i+1,i} (row-major, the records' convention) with a record
// stride; add: blocks subtracted from D (fill a left chunk left in its right separator) or null.  As marginals.hip's MgLevel,
// without everything the backward half needs.
struct EvLevel {
  const double *D, *O, *add;
  int stride, n;
  double *upD, *upO, *upAdd;    // the separators' system: ceil(n / kMgChunk) blocks, upAdd[0] zero (the caller's memset)
  double *part;                 // one sum of log-pivots per chunk
  const double *D0;             // the level-0 records: block i of this level is state i * step of the chain (the pivots' scale)
  int stride0, step;
  int *flag;
};

// In-place Cholesky elimination of the B x W matrix [P | X] (row stride W, P symmetric positive definite in the leading B columns,
// the full square kept): afterwards columns B .. W - 1 hold L^-1 X, P = L L^T.  Returns sum_k log(pivot_k), the same in every
// lane; a pivot that is not positive (flag 1) or below kEvPivotFloor of dref[k], the state's diagonal entry in H (flag 2), counts as
// 1 (the sum stays finite).  One wave; every entry is evaluated from the old matrix, then written (the barriers of a one-wave workgroup)
template <int B, int W> __device__ inline double ev_chol_aug(double *M, const double *dref, int *flag) {
  constexpr int NE = (B * W + 63) / 64;
  double sum = 0.0;
  for (int k = 0; k < B; k++) {     // (not unrolled: with the steps unrolled to skip finished rows B = 12 takes 224 VGPRs and is slower)
    double piv = M[k * W + k];
    if (!(piv > 0.0)) { if (threadIdx.x == 0) *flag = 1; piv = 1.0; }
    else if (!(piv > kEvPivotFloor * dref[k])) { if (threadIdx.x == 0) *flag = 2; piv = 1.0; }     // (positive, below the floor)
    sum += log(piv);
    const double pinv = 1.0 / piv, linv = 1.0 / sqrt(piv);
    double v[NE];
#pragma unroll
    for (int t = 0; t < NE; t++) {
      const int e = threadIdx.x + 64 * t;
      v[t] = 0.0;
      if (e < B * W) {
        const int i = e / W, c = e - i * W;
        const double m = M[e];
        if (i < k || c < k) v[t] = m;                       // rows that are done; the columns of L (never read again)
        else if (i == k) v[t] = m * linv;
        else v[t] = m - M[i * W + k] * M[k * W + c] * pinv;   // (M[i][k] = M[k][i]: the running Schur complement is symmetric)
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NE; t++) {
      const int e = threadIdx.x + 64 * t;
      if (e < B * W) M[e] = v[t];
    }
    __syncthreads();
  }
  return sum;
}

// Eliminate the interiors of one chunk (one wave per chunk), separator s, interiors j = s + 1 .. e - 1, E_j = A_{j,j+1}, F_j = A_{j,s}:
//   P_{s+1} = D_{s+1},  F_{s+1} = A_{s+1,s};   P_j = L L^T,  E^ = L^-1 E_j,  F^ = L^-1 F_j   (ev_chol_aug on [P | E | F]),
//   D_s -= F^^T F^,   P_{j+1} = D_{j+1} - E^^T E^,   F_{j+1} = -E^^T F^;
//   the last interior: D_r -= E^^T E^ (-> upAdd of the right separator), A'_{r,s} = -E^^T F^ (-> upO)
// -- k_mg_forward's recursion with U = P^-1 E, V = P^-1 F never formed.  part[chunk] = sum of log-pivots of the chunk's interiors.
template <int B> __global__ void __launch_bounds__(64) k_ev_forward(EvLevel a) {
  constexpr int BB = B * B, W = 3 * B, NB = (BB + 63) / 64, NP = (3 * BB + 63) / 64;
  __shared__ double M[B * W], Ds[BB], dref[B];
  const int lane = threadIdx.x, k = blockIdx.x, s = k * kMgChunk, e = min(s + kMgChunk, a.n);
  const bool right = e < a.n;
  auto Dg = [&](int i, int idx) { return a.D[(size_t)i * a.stride + idx] - (a.add ? a.add[(size_t)i * BB + idx] : 0.0); };
  auto Og = [&](int i) { return a.O + (size_t)i * a.stride; };
  if (e == s + 1) {                 // a chunk of one state: its coupling to the right separator is the chain's own
    for (int idx = lane; idx < BB; idx += 64) {
      a.upD[(size_t)k * BB + idx] = Dg(s, idx);
      a.upO[(size_t)k * BB + idx] = right ? Og(s)[idx] : 0.0;
    }
    if (lane == 0) a.part[k] = 0.0;
    return;
  }
  for (int idx = lane; idx < BB; idx += 64) {
    const int r = idx / B, c = idx - r * B;
    Ds[idx] = Dg(s, idx);
    M[r * W + c] = Dg(s + 1, idx);
    M[r * W + 2 * B + c] = Og(s)[idx];
  }
  double logsum = 0.0;
  for (int j = s + 1; j < e; j++) {
    const bool hasE = j + 1 < a.n, last = j + 1 == e;
    double dn[NB];                  // D_{j+1}: asked for here, used behind the factorisation
#pragma unroll
    for (int t = 0; t < NB; t++) {
      const int idx = lane + 64 * t;
      dn[t] = 0.0;
      if (idx < BB) {
        const int r = idx / B, c = idx - r * B;
        M[r * W + B + c] = hasE ? Og(j)[c * B + r] : 0.0;     // A_{j,j+1} = O_j^T
        if (!last) dn[t] = Dg(j + 1, idx);
      }
    }
    if (lane < B) dref[lane] = a.D0[(size_t)j * a.step * a.stride0 + lane * (B + 1)];
    __syncthreads();
    logsum += ev_chol_aug<B, W>(M, dref, a.flag);
    double v[NP];
#pragma unroll
    for (int t = 0; t < NP; t++) {
      const int o = lane + 64 * t;
      v[t] = 0.0;
      if (o < 3 * BB) {
        const int which = o / BB, idx = o - which * BB, r = idx / B, c = idx - r * B;
        const double *X = M + (which == 2 ? 2 * B : B) + r, *Y = M + (which == 0 ? B : 2 * B) + c;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < B; q++) acc += X[q * W] * Y[q * W];
        if (which == 0) v[t] = last ? acc : dn[t % NB] - acc;       // (which == 0: o < BB, so t < NB and idx = o)
        else if (which == 1) v[t] = -acc;
        else v[t] = Ds[idx] - acc;
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NP; t++) {
      const int o = lane + 64 * t;
      if (o < 3 * BB) {
        const int which = o / BB, idx = o - which * BB, r = idx / B, c = idx - r * B;
        if (which == 2) Ds[idx] = v[t];
        else if (!last) M[r * W + (which == 0 ? 0 : 2 * B) + c] = v[t];
        else if (which == 1) a.upO[(size_t)k * BB + idx] = v[t];        // (zero without a right separator: E = 0)
        else if (right) a.upAdd[(size_t)(k + 1) * BB + idx] = v[t];
      }
    }
    __syncthreads();
  }
  for (int idx = lane; idx < BB; idx += 64) a.upD[(size_t)k * BB + idx] = Ds[idx];
  if (lane == 0) a.part[k] = logsum;
}

// the top of the recursion: one block, its log-pivots
template <int B> __global__ void __launch_bounds__(64) k_ev_top(EvLevel a) {
  constexpr int BB = B * B;
  __shared__ double M[BB], dref[B];
  for (int idx = threadIdx.x; idx < BB; idx += 64) M[idx] = a.D[idx] - (a.add ? a.add[idx] : 0.0);
  if (threadIdx.x < B) dref[threadIdx.x] = a.D0[threadIdx.x * (B + 1)];      // (the top block is state 0)
  __syncthreads();
  const double sum = ev_chol_aug<B, B>(M, dref, a.flag);
  if (threadIdx.x == 0) a.part[0] = sum;
}

// sum_j log(pivot_j) of the Cholesky elimination of the n x n matrix S (row stride ls, the full square kept), one workgroup of
// kEvCoreThreads; the same in every thread.  A step reads row and column j and writes behind them: one barrier per step
__device__ inline double ev_logdet_n(double *S, int n, int ls, int *flag) {
  double sum = 0.0;
  for (int j = 0; j < n; j++) {
    double dd = S[j * ls + j];
    if (!(dd > 0.0)) { if (threadIdx.x == 0) *flag = 1; dd = 1.0; }
    sum += log(dd);
    const double pinv = 1.0 / dd;
    const int m = n - j - 1;
    for (int idx = threadIdx.x; idx < m * m; idx += kEvCoreThreads) {
      const int i = j + 1 + idx / m, c = j + 1 + idx % m;
      S[i * ls + c] -= S[i * ls + j] * S[j * ls + c] * pinv;
    }
    __syncthreads();
  }
  return sum;
}

// log det(I + 1/2 (U Z + (U Z)^T)) and log det S, one workgroup, the matrix in dynamic LDS (n (n + 1) doubles, n = max(nl, nc)).
// U Z: from the closures' records and the closure columns of the level-0 solution at their two states (one pass: clo_row_dot's
// sums, the block size a runtime number), or from W = U [X | Z] (column passes: columns nr .. nr + nc - 1 of clo.W).  S: lm_S,
// upper part, as k_lm_solve and k_mg_core read it.
struct EvCore {
  const double *S;              // nl x R, columns 1 .. nl
  const double *cloA;           // closure records [A_i | A_j | r]
  const int *first, *second;
  const double *x;              // level-0 solutions N x R x B
  const double *W;              // column passes: nc x ldw, else null
  int ldw, nr;
  int nl, nc, d, R, B;
  double *out;                  // {log det(I + U Z), log det S}
  int *flag;
};
inline size_t ev_core_lds(int n) { return (size_t)std::max(n, 1) * (n + 1) * sizeof(double); }
__global__ void __launch_bounds__(kEvCoreThreads) k_ev_core(EvCore a) {
  extern __shared__ double ev_lds[];
  const int tid = threadIdx.x, nl = a.nl, nc = a.nc, d = a.d, R = a.R;
  double *S = ev_lds;
  double ld_s = 0.0, ld_m = 0.0;
  if (nl > 0) {
    const int ls = nl + 1;
    for (int idx = tid; idx < nl * nl; idx += kEvCoreThreads) {
      const int i = idx / nl, j = idx - i * nl;
      S[i * ls + j] = a.S[(size_t)min(i, j) * R + 1 + max(i, j)];
    }
    __syncthreads();
    ld_s = ev_logdet_n(S, nl, ls, a.flag);
  }
  if (nc > 0) {
    const int ls = nc + 1;
    auto uz = [&](int p, int c) {             // (U Z)[p][c]
      if (a.W) return a.W[(size_t)p * a.ldw + a.nr + c];
      const int kk = p / d, q = p - kk * d;
      const double *rec = a.cloA + (size_t)kk * kCloLen(d);
      const double *xi = a.x + ((size_t)a.first[kk] * R + 1 + nl + c) * a.B, *xj = a.x + ((size_t)a.second[kk] * R + 1 + nl + c) * a.B;
      double acc = 0.0;
      for (int u = 0; u < d; u++) acc += rec[q * d + u] * xi[u];
      for (int u = 0; u < d; u++) acc += rec[d * d + q * d + u] * xj[u];
      return acc;
    };
    for (int idx = tid; idx < nc * nc; idx += kEvCoreThreads) {
      const int p = idx / nc, c = idx - p * nc;
      S[p * ls + c] = clo_sym_entry(p == c, uz(p, c), uz(c, p));
    }
    __syncthreads();
    ld_m = ev_logdet_n(S, nc, ls, a.flag);
  }
  if (tid == 0) { a.out[0] = ld_m; a.out[1] = ld_s; }
}

// res = {log det A, log det(I + U Z), log det S, flag}: the np per-chunk sums of every level in a tree of fixed shape -- thread t adds
// its contiguous run in order, thread 0 the kEvReduceThreads runs in order -- next to k_ev_core's two numbers (res[4], res[5]; zero when
// it did not run) and the pivot flag
__global__ void __launch_bounds__(kEvReduceThreads) k_ev_reduce(const double *part, int np, double *res, const int *flag) {
  __shared__ double red[kEvReduceThreads];
  const int tid = threadIdx.x, per = (np + kEvReduceThreads - 1) / kEvReduceThreads;
  const int i0 = min(tid * per, np), i1 = min(i0 + per, np);
  double acc = 0.0;
  for (int i = i0; i < i1; i++) acc += part[i];
  red[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int t = 0; t < kEvReduceThreads; t++) tot += red[t];
    res[0] = tot; res[1] = res[4]; res[2] = res[5];
    res[3] = (double)*flag;
  }
}

// the refusals of gpslam_hip_log_determinant, before anything is launched
int ev_refuse(gpslam_hip_handle *h, const char *what) {
  const char *why = nullptr;
  if (h->cfg.precision == GPSLAM_FP32) why = "fp32 handles are not supported (fp64 only)";
  else if (sharded(h)) why = "sharded handles are not supported";
  else if (h->fs.active && h->fs.split) why = "split pieces are not supported";
  else if (h->fs.active) why = "the segmented landmark path is not supported (gpslam_hip_marginals_on_segments does not change that)";
  else if (h->mf == ROT3_BIAS) why = "GPSLAM_ROT3_BIAS is not supported (the pad coordinates of its velocity slot are no variables)";
  if (why) return fail(h, GPSLAM_E_UNSUPPORTED, (std::string(what) + ": " + why).c_str());
  return 0;
}

// sum_f log|det R_f|, m, n of the stored graph: host arithmetic over the handle's host copies of the factors
int ev_lognorm(gpslam_hip_handle *h, const char *what, double *lognorm, int64_t *rows, int64_t *vars) {
  auto refuse = [&](const std::string &why) { return fail(h, GPSLAM_E_UNSUPPORTED, (std::string(what) + ": " + why).c_str()); };
  static const char *kind_name[kNumMeasKinds] = {"interpolated range", "range", "interpolated attitude", "interpolated GPS", "odometry",
                                                 "bearing-range", "interpolated projection", "AHRS"};
  if (h->mf == ROT3_BIAS) return refuse("GPSLAM_ROT3_BIAS is not supported (the unit rows on its pad coordinates are no noise model)");
  for (int fk = 0; fk < kNumMeasKinds; fk++) {
    const MeasSet &s = h->ms[fk];
    for (size_t f = 0; 2 * f < s.rob.size(); f++)
      if (s.rob[2 * f] != 0.0)
        return refuse(std::string(kind_name[fk]) + " factor " + std::to_string(f) + " carries a robust loss: the sum of rho is no Gaussian likelihood");
  }
  for (size_t f = 0; 2 * f < h->clo.rob.size(); f++)
    if (h->clo.rob[2 * f] != 0.0) return refuse("loop closure " + std::to_string(f) + " carries a robust loss: the sum of rho is no Gaussian likelihood");
  if (h->sg.count() > 0)
    return refuse("state Gaussian 0 (on state " + std::to_string(h->sg.idx[0]) + "): the constant of a marginalised head was dropped, the window's evidence is not comparable");
  if (h->bg.count() > 0)
    return refuse("border Gaussian 0 (on state " + std::to_string(h->bg.idx[0]) + "): the constant of a marginalised head was dropped, the window's evidence is not comparable");
  if (h->ms[FK_AHRS].count() > 0) return refuse("AHRS factor 0: its rows are whitened by the pre-integrated covariance inside the factor");
  const int d = h->d, b = h->b;
  long double sum = 0.0L;
  int64_t m = 0;
  for (size_t f = 0; f < h->gp_left.size(); f++) {
    const int q = h->gp_q[f];
    const double *Qc = q > 0 ? &h->gp_Qtab[(size_t)(q - 1) * 36] : h->Qc;
    double v = 0.0;
    if (::gpslam_hip_gp_log_normaliser(d, Qc, h->gp_dt[f], &v)) return fail(h, GPSLAM_E_INVALID, "log_noise_normaliser: a stored GP prior has no valid Qc / delta_t");
    sum += v;
    m += b;
  }
  auto diag = [&](const std::vector<double> &sig, int64_t count, int width) {
    for (size_t i = 0; i < (size_t)count * width; i++) sum -= std::log(sig[i]);
    m += count * width;
  };
  diag(h->pri.sig, h->pri.count(), d);
  diag(h->vpri.sig, h->vpri.count(), d);
  diag(h->btw.sig, h->btw.count(), d);
  diag(h->lpri.sig, h->lpri.count(), h->ld);
  diag(h->clo.fac.sig, h->clo.fac.count(), d);
  for (int fk = 0; fk < kNumMeasKinds; fk++) {
    const MeasSet &s = h->ms[fk];
    if (s.count() == 0) continue;
    if (s.sqi.empty()) { diag(s.sig, s.count(), s.rows); continue; }
    // gpslam_hip_set_meas_covariance: R = chol_upper(cov^-1) per factor (diag(1 / sigma) where the factor kept its sigmas), so
    // log|det R| = sum log R_rr = -1/2 log det cov
    for (size_t i = 0; i < (size_t)s.count() * s.rows; i++) sum += std::log(s.sqi[(i / s.rows) * s.rows * s.rows + (i % s.rows) * (s.rows + 1)]);
    m += (int64_t)s.count() * s.rows;
  }
  *lognorm = (double)sum;
  if (rows) *rows = m;
  if (vars) *vars = (int64_t)h->N * b + (int64_t)h->L * h->ld;
  return 0;
}

int ev_logdet(gpslam_hip_handle *h, double *logdet, double *parts3) {
  int rc;
  (void)hipSetDevice(h->cfg.device);
  h->mg.invalidate();             // the solver's buffers, which the marginals' getters read, are rewritten below
  const int N = h->N, B = h->b, BB = B * B, R = h->R, m = R - 1;
  const MgLevels lv(N, B);        // (its n[] and top: the partition; the slabs here hold three blocks per separator, not eight)
  const int top = lv.top;
  size_t uoff[kMgMaxLevels + 1], poff[kMgMaxLevels + 1];
  uoff[0] = uoff[1] = 0; poff[0] = 0;
  for (int l = 1; l <= top; l++) { uoff[l + 1] = uoff[l] + 3 * (size_t)BB * lv.n[l]; poff[l] = poff[l - 1] + lv.n[l]; }
  const int np = (int)poff[top] + 1;
  h->evd.fit(N);
  HIPCHK(h->evd.up.reserve(std::max<size_t>(uoff[top + 1], 1) * sizeof(double)));
  HIPCHK(h->evd.part.reserve((size_t)np * sizeof(double)));
  HIPCHK(h->evd.res.reserve(6 * sizeof(double)));
  const bool passes = h->clo.P > 1;
  const int nc = h->clo.n > 0 ? h->clo.nc : 0, nl = h->nl, ncore = std::max(nc, nl);
  // (process-wide per kernel and device: always the size of the widest system, asked for once)
  static std::atomic<uint64_t> core_lds_set{0};
  const uint64_t dev_bit = h->cfg.device < 64 ? uint64_t(1) << h->cfg.device : 0;
  if (ncore > 0 && !(core_lds_set.load() & dev_bit)) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ev_core), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ev_core_lds(kCloWideMax)));
    core_lds_set.fetch_or(dev_bit);
  }
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  HIPCHK(hipMemsetAsync(h->evd.res.p, 0, 6 * sizeof(double), h->stream));
  if ((rc = impl64::launch_factors(h, LaunchMode{}, 0, 0)) || (rc = impl64::launch_assemble(h, LaunchMode{}, false))) return rc;
  const double *blk = h->lv[0].blk.as<double>();
  double *up = h->evd.up.as<double>(), *part = h->evd.part.as<double>(), *res = h->evd.res.as<double>();
  auto level = [&](int l) {
    EvLevel a;
    if (l == 0) { a.D = blk; a.O = blk + BB; a.add = nullptr; a.stride = 2 * BB + B * R; }
    else { a.D = up + uoff[l]; a.O = a.D + (size_t)BB * lv.n[l]; a.add = a.O + (size_t)BB * lv.n[l]; a.stride = BB; }
    a.n = lv.n[l];
    a.upD = a.upO = a.upAdd = nullptr;          // (unused on the top level)
    if (l < top) { a.upD = up + uoff[l + 1]; a.upO = a.upD + (size_t)BB * lv.n[l + 1]; a.upAdd = a.upO + (size_t)BB * lv.n[l + 1]; }
    a.part = part + (l < top ? poff[l] : poff[top]);
    a.D0 = blk; a.stride0 = 2 * BB + B * R; a.step = 1;
    for (int q = 0; q < l; q++) a.step *= kMgChunk;
    a.flag = h->flag.as<int>();
    return a;
  };
  // (b) reads D / O of the records before the solver below factors them in place
  for (int l = 0; l < top; l++) {
    const EvLevel a = level(l);
    HIPCHK(hipMemsetAsync(a.upAdd, 0, (size_t)BB * sizeof(double), h->stream));
    dispatch_b(B, [&](auto tag) { k_ev_forward<decltype(tag)::value><<<dim3(lv.n[l + 1]), dim3(64), 0, h->stream>>>(a); });
  }
  dispatch_b(B, [&](auto tag) { k_ev_top<decltype(tag)::value><<<dim3(1), dim3(64), 0, h->stream>>>(level(top)); });
  HIPCHK(hipGetLastError());
  // (c) landmarks and closures
  if (m > 0) {
    LaunchMode border;
    border.lm_reduce_only = true;   // (no kept Z: in column passes W = U [X | Z] in clo.W is all k_ev_core reads)
    if ((rc = impl64::launch_solve(h, border, 0.0))) return rc;
    EvCore c;
    c.S = h->lm_S.as<double>(); c.cloA = h->clo.A.as<double>(); c.first = h->clo.fac.d_idx.as<int>(); c.second = h->clo.d_second.as<int>();
    c.x = h->lv[0].x.as<double>(); c.W = passes ? h->clo.W.as<double>() : nullptr; c.ldw = clo_ldw(h); c.nr = 1 + nl;
    c.nl = nl; c.nc = nc; c.d = h->d; c.R = R; c.B = B;
    c.out = res + 4; c.flag = h->flag.as<int>();
    k_ev_core<<<dim3(1), dim3(kEvCoreThreads), ev_core_lds(ncore), h->stream>>>(c);
  }
  k_ev_reduce<<<dim3(1), dim3(kEvReduceThreads), 0, h->stream>>>(part, np, res, h->flag.as<int>());
  HIPCHK(hipGetLastError());
  double out[4];
  HIPCHK(hipMemcpyAsync(out, res, sizeof(out), hipMemcpyDeviceToHost, h->stream));   // the one read: three parts and the flag
  HIPCHK(hipStreamSynchronize(h->stream));
  if (out[3] == 2.0)
    return fail(h, GPSLAM_E_NOT_SPD, "log_determinant: a pivot of the chain's elimination is below 2^-36 of its coordinate's diagonal entry in H, nothing of it is "
                "significant (an indeterminate system: is the graph anchored? -- or a Jacobi-scaled condition number beyond about 7e10)");
  if (out[3] != 0.0) return fail(h, GPSLAM_E_NOT_SPD, "log_determinant: non-positive pivot (indeterminate system: is the graph anchored?)");
  if (parts3) { parts3[0] = out[0]; parts3[1] = out[1]; parts3[2] = out[2]; }
  *logdet = (out[0] + out[1]) + out[2];
  return 0;
}

}  // namespace

extern "C" {

int gpslam_hip_gp_log_normaliser(int32_t d, const double *Qc, double dt, double *out) {
  if (d < 1 || d > 6 || !Qc || !out || !(dt > 0.0) || !std::isfinite(dt)) return GPSLAM_E_INVALID;
  double C[36];
  for (int i = 0; i < d * d; i++) {
    if (!std::isfinite(Qc[i])) return GPSLAM_E_INVALID;
    C[i] = Qc[i];
  }
  if (!spd_chol_upper(d, C)) return GPSLAM_E_INVALID;       // Qc = C^T C (the upper triangle, as gpslam_hip_set_qc reads it)
  double logdet_qc = 0.0;
  for (int i = 0; i < d; i++) logdet_qc += 2.0 * std::log(C[i * d + i]);
  // det Q(dt) = det [[dt^3 / 3, dt^2 / 2], [dt^2 / 2, dt]]^d  det(Qc)^2 = (dt^4 / 12)^d det(Qc)^2
  *out = -0.5 * ((double)d * (4.0 * std::log(dt) - std::log(12.0)) + 2.0 * logdet_qc);
  return 0;
}

int gpslam_hip_evidence_combine(double cost, double logdet, double lognorm, int64_t rows, int64_t vars, double *logZ) {
  if (!logZ) return GPSLAM_E_INVALID;
  constexpr double kLog2Pi = 1.8378770664093454835606594728112;
  *logZ = -cost + lognorm - 0.5 * logdet - 0.5 * (double)(rows - vars) * kLog2Pi;
  return 0;
}

int gpslam_hip_log_determinant(gpslam_hip_handle *h, double *logdet, double *parts3) {
  int rc = need_compiled(h);
  if (rc) return rc;
  if (!logdet) return GPSLAM_E_INVALID;
  if ((rc = ev_refuse(h, "log_determinant"))) return rc;
  return ev_logdet(h, logdet, parts3);
}

int gpslam_hip_log_noise_normaliser(gpslam_hip_handle *h, double *lognorm, int64_t *rows, int64_t *vars) {
  if (!h || !lognorm) return GPSLAM_E_INVALID;
  return ev_lognorm(h, "log_noise_normaliser", lognorm, rows, vars);
}

int gpslam_hip_log_evidence(gpslam_hip_handle *h, double *out5) {
  int rc = need_compiled(h);
  if (rc) return rc;
  if (!out5) return GPSLAM_E_INVALID;
  double lognorm = 0.0, cost = 0.0, logdet = 0.0;
  int64_t rows = 0, vars = 0;
  // every refusal first: nothing is launched on a graph that has no evidence
  if ((rc = ev_refuse(h, "log_evidence")) || (rc = ev_lognorm(h, "log_evidence", &lognorm, &rows, &vars))) return rc;
  if ((rc = ::gpslam_hip_error(h, &cost))) return rc;
  if ((rc = ev_logdet(h, &logdet, nullptr))) return rc;
  out5[1] = cost; out5[2] = logdet; out5[3] = lognorm; out5[4] = (double)(rows - vars);
  return ::gpslam_hip_evidence_combine(cost, logdet, lognorm, rows, vars, &out5[0]);
}

}  // extern "C"
