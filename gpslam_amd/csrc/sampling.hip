// sampling.hip -- draws from the Laplace posterior N(x^, H^-1) by perturbed solves (include/gpslam_hip_sampling.h):
//   delta(eps) = -H^-1 J^T eps,  eps ~ N(0, I) one entry per whitened row,  cov delta = H^-1 J^T J H^-1 = H^-1
// -- the Gauss-Newton step the graph would take if every whitened residual were eps.  fp64, unsharded handles with the dense landmark
// border (or none), no closures, no state or border Gaussians (ps_guard).
//
// Per call: ONE linearisation with every GP prior in the row tables (LaunchMode::d3_rows), the whitened errors of the tables saved, a
// scratch copy of the landmark priors' measurements put in the handle's place.  Per draw: k_ps_place writes a staged noise row where
// the assembly and the landmark reduction read residuals (rowE, rowCE; the scratch priors hold l - sigma eps, so that the
// k_lm_* family's (l - prior) / sigma^2 is eps / sigma) -> launch_assemble -> launch_solve (lambda = 0, level 0 unfused) -> k_ps_emit
// gathers delta from column 0 of the level-0 solution and lm_dL and writes x^ (+) delta into the output slabs; the estimate is only read.
// Per chunk of draws: k_ps_noise (or one copy of the caller's noise) in front, one read of the pivot flag and of the slabs behind.
// At the end the tables' errors and the priors are put back.
//
// Draws at query times (include/gpslam_hip_sampling_at.h): the same loop with an optional part (PsAt).  The
// staged noise rows are n_noise_at wide -- k_ps_noise writes the bridge's normals behind the rows', one kernel and one arithmetic for
// both -- the pose and velocity slabs are kept whether or not the caller asks for them, and ONE k_ps_bridge launch per chunk, behind
// the chunk's last k_ps_emit, walks every run of queries of every draw of the chunk from that draw's own support states in the slabs.
//
// Statistics of those draws (include/gpslam_hip_sampling_stats.h): a second optional part (PsStats) behind the
// first.  Once per call k_interp_query writes q^ of every query; per chunk k_ps_moments, behind the chunk's k_ps_bridge, walks the
// chunk's draws of each query in order out of the query slab -- local coordinates around q^ into the running sums, clearances and
// segment lengths into two draws x queries slabs -- and k_ps_paths reduces those slabs, a workgroup per draw and tile of queries and
// level after level, to one clearance and one length per draw.  No
// query slab goes to the host: per chunk the draws' clearances and lengths, at the end of the call the per-query sums.
#include "api_common.hpp"
#include "../../include/gpslam_hip_sampling_stats.h"

#include <cmath>

namespace impl64 {
#include "api_decl.inc"
}

namespace {

// doubles per staging / output slab at most (32 MiB): a chunk of draws is as many as fit, at least one
// (tests/test_gpu_sampling_at.py restates this number and ps_chunk's rule as KSLAB to pick a call that spans two chunks: keep them in step)
constexpr size_t kPsSlab = size_t(1) << 22;

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3; SC'11), the key bumped before every
// round but the first
__device__ __forceinline__ void ps_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the standard normal of (seed, sample s, noise index j): the header's formula, one normal per counter
__device__ __forceinline__ double ps_normal(uint64_t seed, uint64_t s, uint64_t j) {
  uint32_t w[4];
  ps_philox((uint32_t)j, (uint32_t)(j >> 32), (uint32_t)s, (uint32_t)(s >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
  constexpr double k32 = 0x1p-32, kTwoPi = 6.283185307179586476925286766559;
  const double u1 = ((double)w[0] + ((double)w[1] + 0.5) * k32) * k32;      // in (0, 1]
  const double u2 = ((double)w[2] + (double)w[3] * k32) * k32;              // in [0, 1]
  return sqrt(-2.0 * log(u1)) * cos(kTwoPi * u2);
}

// out[k * n_noise + j] = the normal of sample first + k, noise index j; one thread per entry
__global__ void __launch_bounds__(256) k_ps_noise(uint64_t seed, uint64_t first, int count, int n_noise, double *out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)count * n_noise) return;
  const size_t k = i / (size_t)n_noise, j = i - k * (size_t)n_noise;
  out[i] = ps_normal(seed, first + k, j);
}

struct PsPlace {
  const double *eps;        // one staged row: [M full-width rows | Mc compact rows | npri x ld landmark-prior coordinates]
  int M, Mc, npri, ld;
  double *rowE, *rowCE;     // the tables' whitened errors
  const int *pri_lm;
  const double *pri_sig, *lmk;
  double *pri;              // the scratch priors: l - sigma eps
};
// one thread per noise entry
__global__ void __launch_bounds__(256) k_ps_place(PsPlace a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.M) a.rowE[i] = a.eps[i];
  else if (i < a.M + a.Mc) a.rowCE[i - a.M] = a.eps[i];
  else if (i < a.M + a.Mc + a.npri * a.ld) {
    const int e = i - a.M - a.Mc, k = e / a.ld, q = e - k * a.ld;
    a.pri[e] = a.lmk[(size_t)a.pri_lm[k] * a.ld + q] - a.pri_sig[e] * a.eps[i];
  }
}

struct PsEmit {
  const double *x;          // level-0 solution, N x R x b: column 0 is the step
  const double *dL;         // lm_dL (nl) or null
  const double *pose, *vel, *lmk;   // the estimate: read, never written
  int N, R, stride, chart, nl;
  int pad0;                 // coordinates pad0 .. b - 1 of a block are pads (GPSLAM_ROT3_BIAS: 9), or b
  // this draw's rows of the output slabs; any may be null
  double *delta;            // N * b + nl
  double *poses, *vels;     // N x pd, N x d: the layout of gpslam_hip_get_states
  double *lms;              // nl: the layout of gpslam_hip_get_landmarks
};
// Threads 0 .. N - 1: one state each -- its block of delta (pads an exact 0) and x^_i (+) delta_i by the manifold's own retraction
// (k_retract's arithmetic, into the slab instead of the estimate); threads N .. N + nl - 1: one landmark coordinate each
template <int MF> __global__ void __launch_bounds__(128) k_ps_emit(PsEmit a) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, b = 2 * d;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.N) {
    const double *dl = a.x + (size_t)i * a.R * b;
    double dlt[b], x[pd], out[pd];
#pragma unroll
    for (int k = 0; k < b; k++) dlt[k] = (k >= a.pad0) ? 0.0 : dl[k];
    if (a.delta) {
#pragma unroll
      for (int k = 0; k < b; k++) a.delta[(size_t)i * b + k] = dlt[k];
    }
    if (a.poses) {
#pragma unroll
      for (int k = 0; k < pd; k++) x[k] = a.pose[(size_t)k * a.stride + i];
      PoseFactors<double, MF, false>::retract(x, dlt, a.chart, out);
#pragma unroll
      for (int k = 0; k < pd; k++) a.poses[(size_t)i * pd + k] = out[k];
    }
    if (a.vels) {
#pragma unroll
      for (int k = 0; k < d; k++) a.vels[(size_t)i * d + k] = a.vel[(size_t)k * a.stride + i] + dlt[d + k];
    }
  } else if (i < a.N + a.nl) {
    const int j = i - a.N;
    const double v = a.dL[j];
    if (a.delta) a.delta[(size_t)a.N * b + j] = v;
    if (a.lms) a.lms[j] = a.lmk[j] + v;
  }
}

// doubles per query of the bridge's coefficient table: the first block rows of Lambda_k, Psi_k (l11, l12, p11, p12), the second
// (l21, l22, p21, p22), and the Cholesky factor of K (l00, l10, l11)
constexpr int kPsCoef = 11;

struct PsBridge {
  const double *poses, *vels;       // the chunk's support slabs: draws x N x pd, draws x N x d (what k_ps_emit wrote)
  const double *eps;                // the chunk's staged noise rows, ldn wide; a draw's bridge normals start at column n_noise
  const int *run_ptr, *run_left;    // CSR over runs: queries run_ptr[r] .. run_ptr[r + 1] - 1 lie in interval run_left[r]
  const double *coef;               // nq x kPsCoef
  int N, draws, nruns, nq, n_noise, ldn;
  double Lq[21];                    // the lower Cholesky factor of Qc, rows packed: entry (r, c) at r (r + 1) / 2 + c
  double *qposes, *qvels;           // the chunk's query slabs: draws x nq x pd, draws x nq x d (null: not asked for)
};

// the local variable of an interval and the way back: xb = xi(t_i+1), xdb = J v_i+1 (J = Jr^-1(xb) on SE(3), I elsewhere: the
// interpolators' own arithmetic, factors.hpp interp_pose2 / interp_rot3 / interp_pose3), and put = T_i (+) Exp(xi)
template <int MF> struct PsLocal;
template <int D> struct PsLocalLinear {
  static __device__ __forceinline__ void ends(const double *p1, const double *p2, const double *v2, double *xb, double *xdb) {
#pragma unroll
    for (int c = 0; c < D; c++) { xb[c] = p2[c] - p1[c]; xdb[c] = v2[c]; }
  }
  static __device__ __forceinline__ void put(const double *p1, const double *xi, double *o) {
#pragma unroll
    for (int c = 0; c < D; c++) o[c] = p1[c] + xi[c];
  }
};
template <> struct PsLocal<LINEAR2> : PsLocalLinear<2> {};
template <> struct PsLocal<LINEAR3> : PsLocalLinear<3> {};
template <> struct PsLocal<POSE2> {
  static __device__ __forceinline__ void ends(const double *p1, const double *p2, const double *v2, double *xb, double *xdb) {
    const SE2<double> a = {p1[0], p1[1], p1[2]}, b = {p2[0], p2[1], p2[2]};
    const V3<double> r = se2_log(se2_between(a, b));
    xb[0] = r.x; xb[1] = r.y; xb[2] = r.z;
#pragma unroll
    for (int c = 0; c < 3; c++) xdb[c] = v2[c];
  }
  static __device__ __forceinline__ void put(const double *p1, const double *xi, double *o) {
    const SE2<double> a = {p1[0], p1[1], p1[2]};
    const SE2<double> r = se2_compose(a, se2_exp(V3<double>{xi[0], xi[1], xi[2]}));
    o[0] = r.x; o[1] = r.y; o[2] = r.th;
  }
};
template <> struct PsLocal<ROT3> {
  static __device__ __forceinline__ void ends(const double *p1, const double *p2, const double *v2, double *xb, double *xdb) {
    const V3<double> r = so3_log(transpose(as_m3(p1)) * as_m3(p2));
    xb[0] = r.x; xb[1] = r.y; xb[2] = r.z;
#pragma unroll
    for (int c = 0; c < 3; c++) xdb[c] = v2[c];
  }
  static __device__ __forceinline__ void put(const double *p1, const double *xi, double *o) {
    const M3<double> r = as_m3(p1) * so3_exp(V3<double>{xi[0], xi[1], xi[2]});
#pragma unroll
    for (int c = 0; c < 9; c++) o[c] = r.m[c];
  }
};
template <> struct PsLocal<POSE3> {
  static __device__ __forceinline__ void ends(const double *p1, const double *p2, const double *v2, double *xb, double *xdb) {
    const V6<double> r = se3_log(se3_between(as_se3(p1), as_se3(p2)));
    const V6<double> jv = se3_jrinv_k(jr_coefs(r.w), r) * as_v6(v2);
    xb[0] = r.w.x; xb[1] = r.w.y; xb[2] = r.w.z; xb[3] = r.v.x; xb[4] = r.v.y; xb[5] = r.v.z;
    xdb[0] = jv.w.x; xdb[1] = jv.w.y; xdb[2] = jv.w.z; xdb[3] = jv.v.x; xdb[4] = jv.v.y; xdb[5] = jv.v.z;
  }
  static __device__ __forceinline__ void put(const double *p1, const double *xi, double *o) {
    const SE3<double> r = se3_compose(as_se3(p1), se3_exp(as_v6(xi)));
#pragma unroll
    for (int c = 0; c < 9; c++) o[c] = r.R.m[c];
    o[9] = r.t.x; o[10] = r.t.y; o[11] = r.t.z;
  }
};

// One work item per (draw of the chunk, run of queries): the draw's two support states of the run's interval from the slabs, the
// interval's local variable once, then the walk over the run's queries in order
//   gamma_k = Lambda_k gamma_k-1 + Psi_k gamma(t_i+1) + [l00 Lq eps_p; l10 Lq eps_p + l11 Lq eps_v]
// and T_i (+) Exp(xi_k) per query into the query slab.  Neighbouring work items are neighbouring runs of one draw.  No atomics.
// A work item's records (eleven coefficients and 2 d normals read, pose_dim doubles written per query) lie a whole run from its
// neighbour's.  Measured: that costs bandwidth from four queries per run on, and staging the workgroup's
// queries through LDS in tiles of 128 -- copies in and out with consecutive lanes on consecutive doubles -- was 1.5 to 2.6 times
// SLOWER at 1e6 SE(3) states: a tile of 128 queries holds 128 / m runs of m queries, so 1 / m of the lanes walk while the rest wait at
// the tile's barriers.  The direct form stays.
template <int MF> __global__ void __launch_bounds__(128) k_ps_bridge(PsBridge a) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)a.draws * a.nruns) return;
  const int k = (int)(t / (size_t)a.nruns), run = (int)(t - (size_t)k * a.nruns);
  const int i = a.run_left[run], q1 = a.run_ptr[run + 1];
  const double *P = a.poses + ((size_t)k * a.N + i) * pd, *V = a.vels + ((size_t)k * a.N + i) * d;
  double p1[pd], xb[d], xdb[d], xi[d], xd[d];
  {
    double p2[pd], v2[d];
#pragma unroll
    for (int c = 0; c < pd; c++) { p1[c] = P[c]; p2[c] = P[pd + c]; }
#pragma unroll
    for (int c = 0; c < d; c++) { xi[c] = 0.0; xd[c] = V[c]; v2[c] = V[d + c]; }     // gamma_0 = [0; v_i]
    PsLocal<MF>::ends(p1, p2, v2, xb, xdb);
  }
  const double *eps = a.eps + (size_t)k * a.ldn + a.n_noise;
  for (int q = a.run_ptr[run]; q < q1; q++) {
    const double *cf = a.coef + (size_t)q * kPsCoef, *e = eps + (size_t)q * (2 * d);
    const double l11 = cf[0], l12 = cf[1], p11 = cf[2], p12 = cf[3], l21 = cf[4], l22 = cf[5], p21 = cf[6], p22 = cf[7];
    const double c00 = cf[8], c10 = cf[9], c11 = cf[10];
    double ep[d], ev[d];
#pragma unroll
    for (int c = 0; c < d; c++) { ep[c] = e[c]; ev[c] = e[d + c]; }
#pragma unroll
    for (int r = 0; r < d; r++) {
      double wp = 0.0, wv = 0.0;
#pragma unroll
      for (int c = 0; c <= r; c++) { wp += a.Lq[r * (r + 1) / 2 + c] * ep[c]; wv += a.Lq[r * (r + 1) / 2 + c] * ev[c]; }
      const double x0 = xi[r], x1 = xd[r];
      xi[r] = l11 * x0 + l12 * x1 + p11 * xb[r] + p12 * xdb[r] + c00 * wp;
      xd[r] = l21 * x0 + l22 * x1 + p21 * xb[r] + p22 * xdb[r] + c10 * wp + c11 * wv;
    }
    const size_t at = (size_t)k * a.nq + q;
    double o[pd];
    PsLocal<MF>::put(p1, xi, o);
#pragma unroll
    for (int c = 0; c < pd; c++) a.qposes[at * pd + c] = o[c];
    if (a.qvels) {
#pragma unroll
      for (int c = 0; c < d; c++) a.qvels[at * d + c] = xd[c];
    }
  }
}

// where a pose's position sits in its row (gpslam_hip_sampling_stats.h): the first two coordinates, or the translation of SE(3)
template <int MF> struct PsPos {
  static constexpr int w = MF == POSE3 ? 3 : 2, at = MF == POSE3 ? 9 : 0;
};

// a pose row out of a slab: 16-byte loads where every row starts on 16 bytes (an even pose_dim), 8-byte loads elsewhere
template <int PD> __device__ __forceinline__ void ps_row(const double *p, double *x) {
  if constexpr (PD % 2 == 0) {
#pragma unroll
    for (int c = 0; c < PD; c += 2) {
      const double2 v = *reinterpret_cast<const double2 *>(p + c);
      x[c] = v.x; x[c + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int c = 0; c < PD; c++) x[c] = p[c];
  }
}

struct PsMoments {
  const double *qposes;     // the chunk's query slab: draws x nq x pd (what k_ps_bridge wrote)
  const double *ref;        // nq x pd: q^, the interpolated estimate
  const double *obs;        // n_obs x (w + 1): centre, radius
  int draws, nq, chart, n_obs;
  double margin;
  double *s1, *s2;          // the running sums, nq x d and nq x d (d + 1) / 2 (rows packed as PsBridge::Lq); both or neither
  long long *hits;          // nq, or null
  bool need_g;              // clearances wanted (for hits or for gslab)
  double *gslab, *lslab;    // draws x nq: g_kq and |p_k,q+1 - p_k,q| (0 behind the last query); either may be null
};
// One work item per query: q^ and the query's sums in registers, the chunk's draws in order k = 0, 1, ... -- so a sum is the same
// number however the call is cut into chunks or continued -- and no atomics: every sum has one owner.
template <int MF> __global__ void __launch_bounds__(128) k_ps_moments(PsMoments a) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, T = d * (d + 1) / 2;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.nq) return;
  const bool mom = a.s1 != nullptr;
  double ref[pd], s1[d], s2[T];
  long long hits = a.hits ? a.hits[q] : 0;
  if (mom) ps_row<pd>(a.ref + (size_t)q * pd, ref);
#pragma unroll
  for (int c = 0; c < d; c++) s1[c] = mom ? a.s1[(size_t)q * d + c] : 0.0;
#pragma unroll
  for (int c = 0; c < T; c++) s2[c] = mom ? a.s2[(size_t)q * T + c] : 0.0;
  for (int k = 0; k < a.draws; k++) {
    const size_t at = (size_t)k * a.nq + q;
    const double *P = a.qposes + at * pd;
    double x[pd];
    ps_row<pd>(P, x);
    if (mom) {
      double eta[d], Hd[1];
      PoseFactors<double, MF, false>::prior(ref, x, a.chart, eta, Hd);     // Local(q^, q) in the handle's chart
#pragma unroll
      for (int r = 0; r < d; r++) {
        s1[r] += eta[r];
#pragma unroll
        for (int c = 0; c <= r; c++) s2[r * (r + 1) / 2 + c] += eta[r] * eta[c];
      }
    }
    if constexpr (MF != ROT3) {
      constexpr int w = PsPos<MF>::w, p0 = PsPos<MF>::at;
      if (a.need_g) {
        double g = INFINITY;
        for (int o = 0; o < a.n_obs; o++) {
          const double *ob = a.obs + (size_t)o * (w + 1);
          double r2 = 0.0;
#pragma unroll
          for (int c = 0; c < w; c++) { const double dx = x[p0 + c] - ob[c]; r2 += dx * dx; }
          g = fmin(g, sqrt(r2) - ob[w]);
        }
        g -= a.margin;
        if (a.gslab) a.gslab[at] = g;
        if (g < 0.0) hits++;
      }
      if (a.lslab) {
        double len = 0.0;
        if (q + 1 < a.nq) {
          double r2 = 0.0;
#pragma unroll
          for (int c = 0; c < w; c++) { const double dx = P[pd + p0 + c] - x[p0 + c]; r2 += dx * dx; }
          len = sqrt(r2);
        }
        a.lslab[at] = len;
      }
    }
  }
  if (mom) {
#pragma unroll
    for (int c = 0; c < d; c++) a.s1[(size_t)q * d + c] = s1[c];
#pragma unroll
    for (int c = 0; c < T; c++) a.s2[(size_t)q * T + c] = s2[c];
  }
  if (a.hits) a.hits[q] = hits;
}

// entries of a row that one workgroup of k_ps_paths reduces: 16 per lane
constexpr int kPsTile = 256 * 16;

struct PsPaths {
  const double *gin, *lin;          // draws x width: clearances and segment lengths, or the partial results of the level before
  int width, parts;                 // parts = ceil(width / kPsTile)
  double *gout, *lout;              // draws x parts: with parts == 1 the draws' clearance and length; either pair may be null
};
// One workgroup per (draw, tile of kPsTile entries): lane t takes the tile's entries t, t + 256, ... in ascending order, then a fixed
// tree over the lanes in LDS; the host launches it again over the partial results until one is left per draw.  The tiles are cut
// by the number of queries alone, so the order of every addition is the same wherever the draw sits in a chunk or a call.  (The
// minimum is exact in any order.)  One workgroup per draw was measured first: at 1e6 states a chunk is one draw, and 256 lanes
// walking 16 million entries took 27 ms per slab.
__global__ void __launch_bounds__(256) k_ps_paths(PsPaths a) {
  __shared__ double sm[256], sl[256];
  const int t = threadIdx.x;
  const size_t k = blockIdx.x / (unsigned)a.parts;
  const int p = (int)(blockIdx.x - k * a.parts), q1 = min(a.width, (p + 1) * kPsTile);
  double m = INFINITY, l = 0.0;
  for (int q = p * kPsTile + t; q < q1; q += 256) {
    if (a.gin) m = fmin(m, a.gin[k * a.width + q]);
    if (a.lin) l += a.lin[k * a.width + q];
  }
  sm[t] = m; sl[t] = l;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) { sm[t] = fmin(sm[t], sm[t + s]); sl[t] += sl[t + s]; }
    __syncthreads();
  }
  if (t == 0) {
    if (a.gout) a.gout[k * a.parts + p] = sm[0];
    if (a.lout) a.lout[k * a.parts + p] = sl[0];
  }
}

// every refusal, before anything is launched
int ps_guard(gpslam_hip_handle *h, const char *what) {
  int rc = need_compiled(h);
  if (rc) return rc;
  const char *why = nullptr;
  if (h->cfg.precision != GPSLAM_FP64) why = "an fp32 handle (the perturbed solve and the retraction of a draw are fp64 kernels)";
  else if (h->fs.active && h->fs.split) why = "a piece of a split chain";
  else if (sharded(h)) why = "a sharded handle";
  else if (h->fs.active) why = "the segmented landmark path (the records carry no landmark columns there)";
  else if (h->clo.n > 0) why = "loop closures (they have no rows in the tables: their noise needs a square root of its own)";
  else if (h->sg.count() > 0) why = "state Gaussians (a marginalised head's factors are not sampled yet)";
  else if (h->bg.count() > 0) why = "border Gaussians (they have no rows in the tables: their noise needs a square root of its own)";
  if (why) return fail(h, GPSLAM_E_UNSUPPORTED, (std::string(what) + ": not supported on " + why).c_str());
  (void)hipSetDevice(h->cfg.device);
  return 0;
}

int ps_noise_dim(const gpslam_hip_handle *h) { return h->M + h->Mc + h->lpri.count() * h->ld; }

// the optional part of a call: draws at query times (gpslam_hip_sample_posterior_at).  The runs and the coefficient table are on
// the device (h->ps.at_ptr, at_left, at_coef) before ps_sample is called
struct PsAt {
  int nq, nruns;
  double Lq[21];
  double *qposes, *qvels;   // the caller's outputs; either may be null
};

// the second optional part, with the first only: statistics of the draws at the query times (gpslam_hip_sample_posterior_stats).
// q^, the obstacles and the starting sums are on the device (h->ps.st_ref, st_obs, st_s1, st_s2, st_hits) before ps_sample is called
struct PsStats {
  int n_obs;
  double margin;
  double *s1, *s2;          // the caller's outputs; any may be null (s1 and s2 together)
  int64_t *hits;
  double *clearance, *length;
};

// draws per chunk: the widest slab row decides (with queries: the noise row with the bridge's normals, the query poses)
int ps_chunk(const gpslam_hip_handle *h, int count, const PsAt *at = nullptr) {
  const size_t nq = at ? (size_t)at->nq : 0;
  const size_t widest = std::max<size_t>({(size_t)ps_noise_dim(h) + 2 * (size_t)h->d * nq, (size_t)h->N * h->b + (size_t)h->nl, (size_t)h->N * h->pd,
                                          nq * h->pd, 1});
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)count, kPsSlab / widest));
}

int ps_generate(gpslam_hip_handle *h, uint64_t seed, uint64_t first, int count, int n_noise, double *out) {
  const size_t n = (size_t)count * n_noise;
  k_ps_noise<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream>>>(seed, first, count, n_noise, out);
  HIPCHK(hipGetLastError());
  return 0;
}

// the handle's landmark priors point at the scratch copy while this lives
struct PsPriors {
  gpslam_hip_handle *h;
  bool on = false;
  explicit PsPriors(gpslam_hip_handle *hh) : h(hh) {}
  void swap() { std::swap(h->lpri.d_meas, h->ps.pri); on = !on; }
  ~PsPriors() { if (on) swap(); }
};

struct PsOut {
  double *delta, *poses, *vels, *lms;
};

// the draws, chunk by chunk, over the linearisation in place; at: the queries' part (null: gpslam_hip_sample_posterior, which
// launches what it always launched); st: the statistics' part (null: gpslam_hip_sample_posterior_at, likewise)
int ps_draws(gpslam_hip_handle *h, const LaunchMode &m, int count, uint64_t seed, uint64_t first, const double *noise, const PsOut &o,
             const PsAt *at = nullptr, const PsStats *st = nullptr) {
  int rc;
  const int N = h->N, b = h->b, nl = h->nl, n_noise = ps_noise_dim(h), chunk = ps_chunk(h, count, at);
  const int ldn = n_noise + (at ? 2 * h->d * at->nq : 0);          // a staged noise row
  const bool sp = o.poses || at, sv = o.vels || at;                // the bridge reads a draw's support states from the slabs
  const size_t wd = (size_t)N * b + nl, wp = (size_t)N * h->pd, wv = (size_t)N * h->d;
  const size_t wqp = at ? (size_t)at->nq * h->pd : 0, wqv = at ? (size_t)at->nq * h->d : 0;
  HIPCHK(h->ps.stage.reserve(std::max<size_t>((size_t)chunk * ldn, 1) * sizeof(double)));
  if (o.delta) HIPCHK(h->ps.delta.reserve((size_t)chunk * wd * sizeof(double)));
  if (sp) HIPCHK(h->ps.poses.reserve((size_t)chunk * wp * sizeof(double)));
  if (sv) HIPCHK(h->ps.vels.reserve((size_t)chunk * wv * sizeof(double)));
  if (o.lms && nl > 0) HIPCHK(h->ps.lms.reserve((size_t)chunk * nl * sizeof(double)));
  if (at) HIPCHK(h->ps.at_poses.reserve((size_t)chunk * wqp * sizeof(double)));
  if (at && at->qvels) HIPCHK(h->ps.at_vels.reserve((size_t)chunk * wqv * sizeof(double)));
  PsMoments ma;
  if (st) {
    const size_t slab = (size_t)chunk * at->nq * sizeof(double);
    if (st->clearance) HIPCHK(h->ps.st_g.reserve(slab));
    if (st->length) HIPCHK(h->ps.st_seg.reserve(slab));
    if (st->clearance) HIPCHK(h->ps.st_clear.reserve((size_t)chunk * sizeof(double)));
    if (st->length) HIPCHK(h->ps.st_len.reserve((size_t)chunk * sizeof(double)));
    ma.qposes = h->ps.at_poses.as<double>(); ma.ref = h->ps.st_ref.as<double>(); ma.obs = h->ps.st_obs.as<double>();
    ma.nq = at->nq; ma.chart = h->cfg.chart; ma.n_obs = st->n_obs; ma.margin = st->margin;
    ma.s1 = st->s1 ? h->ps.st_s1.as<double>() : nullptr; ma.s2 = st->s1 ? h->ps.st_s2.as<double>() : nullptr;
    ma.hits = st->hits ? h->ps.st_hits.as<long long>() : nullptr;
    ma.need_g = st->hits || st->clearance;
    ma.gslab = st->clearance ? h->ps.st_g.as<double>() : nullptr; ma.lslab = st->length ? h->ps.st_seg.as<double>() : nullptr;
    // k_ps_paths' partial results, level after level: the first level's behind each other, the second's behind those
    const size_t p1 = (size_t)nblocks(at->nq, kPsTile), p2 = (size_t)nblocks((int)p1, kPsTile);
    if (p1 > 1 && (st->clearance || st->length)) HIPCHK(h->ps.st_part.reserve(2 * (size_t)chunk * (p1 + p2) * sizeof(double)));
  }
  PsPlace pa;
  pa.M = h->M; pa.Mc = h->Mc; pa.npri = h->lpri.count(); pa.ld = h->ld;
  pa.rowE = h->rowE.as<double>(); pa.rowCE = h->rowCE.as<double>();
  pa.pri_lm = h->lpri.d_idx.as<int>(); pa.pri_sig = h->lpri.d_sig.as<double>(); pa.lmk = h->lmk.as<double>();
  pa.pri = h->lpri.d_meas.as<double>();        // (the scratch copy: ps_sample has put it in place)
  PsEmit ea;
  ea.x = h->lv[0].x.as<double>(); ea.dL = nl > 0 ? h->lm_dL.as<double>() : nullptr;
  ea.pose = h->pose.as<double>(); ea.vel = h->vel.as<double>(); ea.lmk = h->lmk.as<double>();
  ea.N = N; ea.R = h->R; ea.stride = h->stride; ea.chart = h->cfg.chart; ea.nl = nl;
  ea.pad0 = h->mf == ROT3_BIAS ? 9 : b;
  PsBridge ba;
  if (at) {
    ba.poses = h->ps.poses.as<double>(); ba.vels = h->ps.vels.as<double>(); ba.eps = h->ps.stage.as<double>();
    ba.run_ptr = h->ps.at_ptr.as<int>(); ba.run_left = h->ps.at_left.as<int>(); ba.coef = h->ps.at_coef.as<double>();
    ba.N = N; ba.nruns = at->nruns; ba.nq = at->nq; ba.n_noise = n_noise; ba.ldn = ldn;
    std::memcpy(ba.Lq, at->Lq, sizeof(ba.Lq));
    ba.qposes = h->ps.at_poses.as<double>(); ba.qvels = at->qvels ? h->ps.at_vels.as<double>() : nullptr;
  }
  for (int k0 = 0; k0 < count; k0 += chunk) {
    const int nk = std::min(chunk, count - k0);
    double *stage = h->ps.stage.as<double>();
    if (noise) {
      if (ldn > 0) HIPCHK(hipMemcpyAsync(stage, noise + (size_t)k0 * ldn, (size_t)nk * ldn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else if (ldn > 0 && (rc = ps_generate(h, seed, first + (uint64_t)k0, nk, ldn, stage))) return rc;
    for (int k = 0; k < nk; k++) {
      pa.eps = stage + (size_t)k * ldn;
      if (n_noise > 0) k_ps_place<<<dim3(nblocks(n_noise, 256)), dim3(256), 0, h->stream>>>(pa);
      if ((rc = impl64::launch_assemble(h, m, false)) || (rc = impl64::launch_solve(h, m, 0.0))) return rc;
      ea.delta = o.delta ? h->ps.delta.as<double>() + (size_t)k * wd : nullptr;
      ea.poses = sp ? h->ps.poses.as<double>() + (size_t)k * wp : nullptr;
      ea.vels = sv ? h->ps.vels.as<double>() + (size_t)k * wv : nullptr;
      ea.lms = (o.lms && nl > 0) ? h->ps.lms.as<double>() + (size_t)k * nl : nullptr;
      dispatch_mf(h->mf, [&](auto tag) { k_ps_emit<decltype(tag)::value><<<dim3(nblocks(N + nl, 128)), dim3(128), 0, h->stream>>>(ea); });
      HIPCHK(hipGetLastError());
    }
    if (at) {
      // the chunk's queries in one launch: draws x runs work items
      ba.draws = nk;
      const unsigned nb = (unsigned)(((size_t)nk * at->nruns + 127) / 128);
      switch (h->mf) {      // (ps_at_guard has refused GPSLAM_ROT3_BIAS)
        case LINEAR2: k_ps_bridge<LINEAR2><<<dim3(nb), dim3(128), 0, h->stream>>>(ba); break;
        case LINEAR3: k_ps_bridge<LINEAR3><<<dim3(nb), dim3(128), 0, h->stream>>>(ba); break;
        case POSE2: k_ps_bridge<POSE2><<<dim3(nb), dim3(128), 0, h->stream>>>(ba); break;
        case ROT3: k_ps_bridge<ROT3><<<dim3(nb), dim3(128), 0, h->stream>>>(ba); break;
        case POSE3: k_ps_bridge<POSE3><<<dim3(nb), dim3(128), 0, h->stream>>>(ba); break;
        default: return fail(h, GPSLAM_E_UNSUPPORTED, "sample_posterior_at: no bridge kernel for this manifold");
      }
      HIPCHK(hipGetLastError());
    }
    if (st) {
      // the chunk's draws into the per-query sums and the two slabs, one work item per query; then the slabs' rows reduced, tile by tile
      ma.draws = nk;
      const unsigned nb = (unsigned)nblocks(at->nq, 128);
      switch (h->mf) {
        case LINEAR2: k_ps_moments<LINEAR2><<<dim3(nb), dim3(128), 0, h->stream>>>(ma); break;
        case LINEAR3: k_ps_moments<LINEAR3><<<dim3(nb), dim3(128), 0, h->stream>>>(ma); break;
        case POSE2: k_ps_moments<POSE2><<<dim3(nb), dim3(128), 0, h->stream>>>(ma); break;
        case ROT3: k_ps_moments<ROT3><<<dim3(nb), dim3(128), 0, h->stream>>>(ma); break;
        case POSE3: k_ps_moments<POSE3><<<dim3(nb), dim3(128), 0, h->stream>>>(ma); break;
        default: return fail(h, GPSLAM_E_UNSUPPORTED, "sample_posterior_stats: no reduction kernel for this manifold");
      }
      HIPCHK(hipGetLastError());
      if (st->clearance || st->length) {
        // level after level until one number per draw is left: the slabs, then partial results in the two halves of st_part by turns
        const size_t p1 = (size_t)nblocks(at->nq, kPsTile);
        double *part[2] = {h->ps.st_part.as<double>(), h->ps.st_part.as<double>() + 2 * (size_t)nk * p1};
        PsPaths ta;
        ta.gin = ma.gslab; ta.lin = ma.lslab; ta.width = at->nq;
        for (int level = 0;; level++) {
          ta.parts = nblocks(ta.width, kPsTile);
          const bool last = ta.parts == 1;
          double *dst = part[level & 1];
          ta.gout = !st->clearance ? nullptr : last ? h->ps.st_clear.as<double>() : dst;
          ta.lout = !st->length ? nullptr : last ? h->ps.st_len.as<double>() : dst + (size_t)nk * ta.parts;
          k_ps_paths<<<dim3((unsigned)((size_t)nk * ta.parts)), dim3(256), 0, h->stream>>>(ta);
          HIPCHK(hipGetLastError());
          if (last) break;
          ta.gin = ta.gout; ta.lin = ta.lout; ta.width = ta.parts;
        }
      }
    }
    // the one read of a chunk: the pivot flag (sticky over the chunk's solves), then the slabs
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (flag) return fail(h, GPSLAM_E_NOT_SPD, "sample_posterior: non-positive pivot in the block elimination (indeterminate system: is the graph anchored?)");
    if (o.delta) HIPCHK(hipMemcpyAsync(o.delta + (size_t)k0 * wd, h->ps.delta.p, (size_t)nk * wd * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (o.poses) HIPCHK(hipMemcpyAsync(o.poses + (size_t)k0 * wp, h->ps.poses.p, (size_t)nk * wp * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (o.vels) HIPCHK(hipMemcpyAsync(o.vels + (size_t)k0 * wv, h->ps.vels.p, (size_t)nk * wv * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (o.lms && nl > 0) HIPCHK(hipMemcpyAsync(o.lms + (size_t)k0 * nl, h->ps.lms.p, (size_t)nk * nl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (at && at->qposes) HIPCHK(hipMemcpyAsync(at->qposes + (size_t)k0 * wqp, h->ps.at_poses.p, (size_t)nk * wqp * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (at && at->qvels) HIPCHK(hipMemcpyAsync(at->qvels + (size_t)k0 * wqv, h->ps.at_vels.p, (size_t)nk * wqv * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (st && st->clearance) HIPCHK(hipMemcpyAsync(st->clearance + k0, h->ps.st_clear.p, (size_t)nk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (st && st->length) HIPCHK(hipMemcpyAsync(st->length + k0, h->ps.st_len.p, (size_t)nk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  if (st) {
    // the per-query sums, once
    const size_t nq = (size_t)at->nq, d = (size_t)h->d;
    if (st->s1) HIPCHK(hipMemcpyAsync(st->s1, h->ps.st_s1.p, nq * d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (st->s1) HIPCHK(hipMemcpyAsync(st->s2, h->ps.st_s2.p, nq * (d * (d + 1) / 2) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (st->hits) HIPCHK(hipMemcpyAsync(st->hits, h->ps.st_hits.p, nq * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int ps_sample(gpslam_hip_handle *h, int count, uint64_t seed, uint64_t first, const double *noise, const PsOut &o, const PsAt *at = nullptr,
              const PsStats *st = nullptr) {
  int rc;
  h->mg.invalidate();             // the solver's buffers, which the marginals' getters read, are rewritten below
  const size_t nE = (size_t)h->M * sizeof(double), nCE = (size_t)h->Mc * sizeof(double);
  const size_t npri = (size_t)h->lpri.count() * h->ld * sizeof(double);
  HIPCHK(h->ps.saveE.reserve(std::max<size_t>(nE + nCE, 8)));
  HIPCHK(h->ps.pri.reserve(std::max<size_t>(npri, 8)));
  // the pivot flag cleared; the rows of the current estimate, every GP prior among them (no structured records: k_ps_place writes
  // the tables' errors, and gp_form consults the mode, so the same mode goes to the assembly)
  LaunchMode m;
  m.d3_rows = true;
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  if ((rc = impl64::launch_factors(h, m, 0, 0))) return rc;
  char *save = h->ps.saveE.as<char>();
  if (nE) HIPCHK(hipMemcpyAsync(save, h->rowE.p, nE, hipMemcpyDeviceToDevice, h->stream));
  if (nCE) HIPCHK(hipMemcpyAsync(save + nE, h->rowCE.p, nCE, hipMemcpyDeviceToDevice, h->stream));
  {
    PsPriors guard(h);            // (back in place on every way out of this block)
    if (npri) guard.swap();
    rc = ps_draws(h, m, count, seed, first, noise, o, at, st);
  }
  // the linearisation's own errors back into the tables: the handle is as a call of gpslam_hip_get_rows leaves it
  if (nE) HIPCHK(hipMemcpyAsync(h->rowE.p, save, nE, hipMemcpyDeviceToDevice, h->stream));
  if (nCE) HIPCHK(hipMemcpyAsync(h->rowCE.p, save + nE, nCE, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return rc;
}

// the generator's numbers for count samples, `width` per sample, to the host
int ps_noise_out(gpslam_hip_handle *h, uint64_t seed, uint64_t first, int count, int width, double *noise) {
  int rc;
  if (width == 0) return 0;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)count, kPsSlab / (size_t)width));
  HIPCHK(h->ps.stage.reserve((size_t)chunk * width * sizeof(double)));
  for (int k0 = 0; k0 < count; k0 += chunk) {
    const int nk = std::min(chunk, count - k0);
    if ((rc = ps_generate(h, seed, first + (uint64_t)k0, nk, width, h->ps.stage.as<double>()))) return rc;
    HIPCHK(hipMemcpyAsync(noise + (size_t)k0 * width, h->ps.stage.p, (size_t)nk * width * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

// n_noise_at = n_noise + 2 d n_queries, or (negative) the refusal of a width that an int32 does not hold
int ps_at_width(gpslam_hip_handle *h, int n_queries, const char *what) {
  const int64_t w = (int64_t)ps_noise_dim(h) + 2 * (int64_t)h->d * n_queries;
  if (w > INT32_MAX) return fail(h, GPSLAM_E_INVALID, (std::string(what) + ": the noise vector of that many queries is longer than 2^31 - 1").c_str());
  return (int)w;
}

// what the bridge refuses on top of ps_guard, before anything is launched
int ps_at_guard(gpslam_hip_handle *h, bool query_vels, const char *what = "sample_posterior_at") {
  const char *why = nullptr;
  bool own_qc = false;
  for (int32_t q : h->gp_q) own_qc = own_qc || q != 0;
  if (h->mf == ROT3_BIAS) why = "GPSLAM_ROT3_BIAS handles (the bias is held over an interval, not interpolated)";
  else if (h->vw) why = "world-frame velocities (velocity_world: the interval's local variable differs)";
  else if (own_qc) why = "GP priors with a Qc of their own (gpslam_hip_add_gp_priors_qc): the bridge's noise is the handle's Qc";
  else if (query_vels && h->mf != LINEAR2 && h->mf != LINEAR3) why = "query_vels on a Lie group (GPSLAM_LINEAR2 / LINEAR3 only, as interpolate_velocities)";
  if (why) return fail(h, GPSLAM_E_UNSUPPORTED, (std::string(what) + ": not supported on " + why).c_str());
  return 0;
}

// the queries checked and cut into runs, the bridge's coefficients of every query and the Cholesky factor of Qc; the tables uploaded
int ps_at_upload(gpslam_hip_handle *h, int nq, const int32_t *left, const double *dt, const double *tau, PsAt &at) {
  if (h->N < 2) return fail(h, GPSLAM_E_INVALID, "sample_posterior_at: interpolation needs at least two states");
  auto bad = [&](int q, const char *msg) { return fail(h, GPSLAM_E_INVALID, ("sample_posterior_at: query " + std::to_string(q) + ": " + msg).c_str()); };
  std::vector<int> ptr, rl;
  std::vector<double> coef((size_t)nq * kPsCoef);
  for (int q = 0; q < nq; q++) {
    if (left[q] < 0 || left[q] > h->N - 2) return bad(q, "interval out of range (0 .. N - 2)");
    if (q > 0 && left[q] < left[q - 1]) return bad(q, "left must be non-decreasing");
    const bool head = q == 0 || left[q] != left[q - 1];
    if (!(dt[q] > 0.0)) return bad(q, "delta_t must be positive");
    if (!head && dt[q] != dt[q - 1]) return bad(q, "delta_t differs within one interval");
    if (!(tau[q] > 0.0) || !(tau[q] < dt[q])) return bad(q, "tau must lie inside (0, delta_t): the ends and extrapolation are not sampled");
    if (!head && !(tau[q] > tau[q - 1])) return bad(q, "tau must increase strictly within one interval");
    if (head) { ptr.push_back(q); rl.push_back(left[q]); }
    // (a, tau, b) = (the query before or 0, tau, dt): Psi = Q(u) Phi(s)^T Q(T)^-1, Lambda = Phi(u) - Psi Phi(T), K = l l^T in closed
    // forms without cancellation (the header has them)
    const double a = head ? 0.0 : tau[q - 1], u = tau[q] - a, s = dt[q] - tau[q], T = dt[q] - a, T2 = T * T, T3 = T2 * T, us = u * s;
    double *c = &coef[(size_t)q * kPsCoef];
    c[0] = s * s * (3.0 * u + s) / T3; c[1] = u * s * s / T2; c[2] = u * u * (u + 3.0 * s) / T3; c[3] = -u * u * s / T2;
    c[4] = -6.0 * us / T3; c[5] = s * (s - 2.0 * u) / T2; c[6] = 6.0 * us / T3; c[7] = u * (u - 2.0 * s) / T2;
    c[8] = us * std::sqrt(us) / std::sqrt(3.0 * T3); c[9] = std::sqrt(3.0) * (s - u) * std::sqrt(us) / (2.0 * T * std::sqrt(T));
    c[10] = 0.5 * std::sqrt(us / T);
  }
  ptr.push_back(nq);
  at.nq = nq; at.nruns = (int)rl.size();
  // Qc = U^T U: L_q = U^T, rows packed
  const int d = h->d;
  double U[36];
  std::memcpy(U, h->Qc, sizeof(double) * d * d);
  if (!spd_chol_upper(d, U)) return fail(h, GPSLAM_E_INVALID, "sample_posterior_at: Qc is not positive definite");
  std::memset(at.Lq, 0, sizeof(at.Lq));
  for (int r = 0; r < d; r++)
    for (int c = 0; c <= r; c++) at.Lq[r * (r + 1) / 2 + c] = U[c * d + r];
  int rc;
  if ((rc = upload(h, h->ps.at_ptr, ptr)) || (rc = upload(h, h->ps.at_left, rl)) || (rc = upload(h, h->ps.at_coef, coef))) return rc;
  return 0;
}

// what the statistics read on the device before the first draw: q^ of every query by the interpolators' own kernel over the
// estimate, the obstacles, and the sums a continued call starts from (zeros otherwise)
int ps_stats_upload(gpslam_hip_handle *h, int nq, const int32_t *left, const double *dt, const double *tau, const PsStats &st,
                    const double *obstacles, bool accumulate) {
  int rc;
  const int d = h->d, pd = h->pd, w = h->mf == POSE3 ? 3 : 2;
  std::vector<double> coef((size_t)nq * 4);
  for (int q = 0; q < nq; q++) interp_coef(dt[q], tau[q], &coef[4 * (size_t)q]);
  std::vector<int> li(left, left + nq);
  if ((rc = upload(h, h->ps.st_left, li)) || (rc = upload(h, h->ps.st_coef, coef))) return rc;
  HIPCHK(h->ps.st_ref.reserve((size_t)nq * pd * sizeof(double)));
  HIPCHK(h->ps.st_obs.reserve(std::max<size_t>((size_t)st.n_obs * (w + 1), 1) * sizeof(double)));
  if (st.n_obs > 0) HIPCHK(hipMemcpyAsync(h->ps.st_obs.p, obstacles, (size_t)st.n_obs * (w + 1) * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const size_t n1 = (size_t)nq * d * sizeof(double), n2 = (size_t)nq * (d * (d + 1) / 2) * sizeof(double), nh = (size_t)nq * sizeof(int64_t);
  if (st.s1) {
    HIPCHK(h->ps.st_s1.reserve(n1));
    HIPCHK(h->ps.st_s2.reserve(n2));
    if (accumulate) {
      HIPCHK(hipMemcpyAsync(h->ps.st_s1.p, st.s1, n1, hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipMemcpyAsync(h->ps.st_s2.p, st.s2, n2, hipMemcpyHostToDevice, h->stream));
    } else {
      HIPCHK(hipMemsetAsync(h->ps.st_s1.p, 0, n1, h->stream));
      HIPCHK(hipMemsetAsync(h->ps.st_s2.p, 0, n2, h->stream));
    }
  }
  if (st.hits) {
    HIPCHK(h->ps.st_hits.reserve(nh));
    if (accumulate) HIPCHK(hipMemcpyAsync(h->ps.st_hits.p, st.hits, nh, hipMemcpyHostToDevice, h->stream));
    else HIPCHK(hipMemsetAsync(h->ps.st_hits.p, 0, nh, h->stream));
  }
  QueryArgs<double> a;
  a.pose = h->pose.as<double>(); a.vel = h->vel.as<double>(); a.stride = h->stride; a.count = nq;
  a.left = h->ps.st_left.as<int>(); a.coef = h->ps.st_coef.as<double>(); a.out = h->ps.st_ref.as<double>(); a.out_H = nullptr;
  a.vw = h->vw;
  dispatch_mf(h->mf, [&](auto tag) { k_interp_query<double, decltype(tag)::value, false><<<dim3(nblocks(nq, 128)), dim3(128), 0, h->stream>>>(a); });
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));      // (the caller's arrays are read)
  return 0;
}

}  // namespace

extern "C" {

int gpslam_hip_sample_posterior_stats(gpslam_hip_handle *h, int32_t count, uint64_t seed, uint64_t first, const double *noise,
                                      int32_t n_queries, const int32_t *left, const double *dt, const double *tau,
                                      int32_t n_obstacles, const double *obstacles, double margin,
                                      int32_t accumulate, int64_t *n_draws,
                                      double *s1, double *s2, int64_t *hits, double *clearance, double *length) {
  if (!h || count <= 0 || n_queries <= 0 || !left || !dt || !tau) return GPSLAM_E_INVALID;
  if (!s1 && !s2 && !hits && !clearance && !length) return GPSLAM_E_INVALID;
  if ((s1 == nullptr) != (s2 == nullptr)) return GPSLAM_E_INVALID;
  if (n_obstacles < 0 || n_obstacles > 1024 || (n_obstacles > 0 && !obstacles)) return GPSLAM_E_INVALID;
  if ((n_obstacles == 0) != (!hits && !clearance)) return GPSLAM_E_INVALID;
  if (!(margin >= 0.0)) return GPSLAM_E_INVALID;
  if ((s1 || hits) && !n_draws) return GPSLAM_E_INVALID;
  if (accumulate && n_draws && *n_draws < 0) return GPSLAM_E_INVALID;
  const char *what = "sample_posterior_stats";
  int rc = ps_guard(h, what);
  if (rc || (rc = ps_at_guard(h, false, what))) return rc;
  if (h->mf == ROT3 && (hits || clearance || length))
    return fail(h, GPSLAM_E_UNSUPPORTED, "sample_posterior_stats: hits, clearance and length are not supported on GPSLAM_ROT3 (a rotation has no position)");
  const int w = h->mf == POSE3 ? 3 : 2;
  for (int o = 0; o < n_obstacles; o++)
    if (!(obstacles[(size_t)o * (w + 1) + w] >= 0.0))
      return fail(h, GPSLAM_E_INVALID, ("sample_posterior_stats: obstacle " + std::to_string(o) + ": the radius must not be negative").c_str());
  if ((rc = ps_at_width(h, n_queries, what)) < 0) return rc;
  PsAt at;
  at.qposes = nullptr; at.qvels = nullptr;
  if ((rc = ps_at_upload(h, n_queries, left, dt, tau, at))) return rc;
  const PsStats st{n_obstacles, margin, s1, s2, hits, clearance, length};
  if ((rc = ps_stats_upload(h, n_queries, left, dt, tau, st, obstacles, accumulate != 0))) return rc;
  if ((rc = ps_sample(h, count, seed, first, noise, PsOut{nullptr, nullptr, nullptr, nullptr}, &at, &st))) return rc;
  if (n_draws) *n_draws = (accumulate ? *n_draws : 0) + count;
  return 0;
}

int gpslam_hip_posterior_moments(int32_t d, int32_t n_queries, int64_t n_draws, const double *s1, const double *s2,
                                 double *mean, double *cov) {
  if (d <= 0 || n_queries < 0 || !s1 || !mean || (cov && !s2)) return GPSLAM_E_INVALID;
  if (n_draws < 1 || (cov && n_draws < 2)) return GPSLAM_E_INVALID;
  const double n = (double)n_draws;
  const int T = d * (d + 1) / 2;
  for (int q = 0; q < n_queries; q++) {
    double *m = mean + (size_t)q * d;
    for (int c = 0; c < d; c++) m[c] = s1[(size_t)q * d + c] / n;
    if (!cov) continue;
    for (int r = 0; r < d; r++)
      for (int c = 0; c <= r; c++) {
        const double v = (s2[(size_t)q * T + r * (r + 1) / 2 + c] - n * m[r] * m[c]) / (n - 1.0);
        cov[((size_t)q * d + r) * d + c] = v;
        cov[((size_t)q * d + c) * d + r] = v;
      }
  }
  return 0;
}

int gpslam_hip_posterior_noise_dim(gpslam_hip_handle *h, int32_t *n_noise) {
  int rc = need_compiled(h);
  if (rc) return rc;
  if (!n_noise) return GPSLAM_E_INVALID;
  *n_noise = (int32_t)ps_noise_dim(h);
  return 0;
}

int gpslam_hip_posterior_noise(gpslam_hip_handle *h, uint64_t seed, uint64_t first, int32_t count, double *noise) {
  if (!h || count <= 0 || !noise) return GPSLAM_E_INVALID;
  int rc = need_local(h);
  if (rc) return rc;
  return ps_noise_out(h, seed, first, count, ps_noise_dim(h), noise);
}

int gpslam_hip_posterior_noise_dim_at(gpslam_hip_handle *h, int32_t n_queries, int32_t *n_noise_at) {
  int rc = need_compiled(h);
  if (rc) return rc;
  if (!n_noise_at || n_queries <= 0) return GPSLAM_E_INVALID;
  if ((rc = ps_at_width(h, n_queries, "posterior_noise_dim_at")) < 0) return rc;
  *n_noise_at = (int32_t)rc;
  return 0;
}

int gpslam_hip_posterior_noise_at(gpslam_hip_handle *h, uint64_t seed, uint64_t first, int32_t count, int32_t n_queries, double *noise) {
  if (!h || count <= 0 || n_queries <= 0 || !noise) return GPSLAM_E_INVALID;
  int rc = need_local(h);
  if (rc) return rc;
  if ((rc = ps_at_width(h, n_queries, "posterior_noise_at")) < 0) return rc;
  return ps_noise_out(h, seed, first, count, rc, noise);
}

int gpslam_hip_sample_posterior_at(gpslam_hip_handle *h, int32_t count, uint64_t seed, uint64_t first, const double *noise,
                                   int32_t n_queries, const int32_t *left, const double *dt, const double *tau,
                                   double *query_poses, double *query_vels,
                                   double *delta, double *poses, double *vels, double *landmarks) {
  if (!h || count <= 0 || n_queries <= 0 || !left || !dt || !tau) return GPSLAM_E_INVALID;
  if (!query_poses && !query_vels && !delta && !poses && !vels && !landmarks) return GPSLAM_E_INVALID;
  int rc = ps_guard(h, "sample_posterior_at");
  if (rc || (rc = ps_at_guard(h, query_vels != nullptr))) return rc;
  if ((rc = ps_at_width(h, n_queries, "sample_posterior_at")) < 0) return rc;
  PsAt at;
  at.qposes = query_poses; at.qvels = query_vels;
  if ((rc = ps_at_upload(h, n_queries, left, dt, tau, at))) return rc;
  return ps_sample(h, count, seed, first, noise, PsOut{delta, poses, vels, landmarks}, &at);
}

int gpslam_hip_sample_posterior(gpslam_hip_handle *h, int32_t count, uint64_t seed, uint64_t first,
                                const double *noise, double *delta, double *poses, double *vels, double *landmarks) {
  if (!h || count <= 0 || (!delta && !poses && !vels && !landmarks)) return GPSLAM_E_INVALID;
  int rc = ps_guard(h, "sample_posterior");
  if (rc) return rc;
  return ps_sample(h, count, seed, first, noise, PsOut{delta, poses, vels, landmarks});
}

}  // extern "C"
