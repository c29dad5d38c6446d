// meas_noise.hip -- learning measurement noise from data (include/gpslam_hip_noise.h): per measurement kind
//   B = sum_m (e_m e_m^T + J_m Sigma_m J_m^T),   Bw = sum_m R_m (e_m e_m^T + J_m Sigma_m J_m^T) R_m^T,   n = the factors summed,
// from what gpslam_hip_marginals left on the device (mg.S, mg.Sn, mg.Sxl, mg.Slm) and the factors' own unwhitened e and
// J = [H1 H2 | H3 H4 | H5] (k_meas's inspection mode through launch_meas_inspect: the factor maths is not restated here), the
// per-factor P_m = J_m Sigma_m J_m^T, and the host arithmetic on the statistic: G = 1/2 (n C - B), C+ = B / n, theta+ / theta.
//   (a) the kind's factors go in chunks of a fixed slab of e / J scratch (api_e, api_H: what gpslam_hip_linearize_meas writes), each
//       chunk evaluated by launch_meas_inspect and contracted by one launch of
//   (b) k_mn_stat<B, LD, ROWS, TWO, HASLM>: one wave per workgroup, a contiguous run of the chunk's factors in an order sorted by left
//       state (a stable sort, built on the host once per compile()).  Per factor the wave lays Sigma_m out in LDS -- S_i, Sn_i, S_{i+1}
//       as whole coalesced blocks, only when the interval differs from the previous factor's; the landmark's b x ld columns of Sxl and
//       its ld x ld block of Slm -- and J, e and R next to it; everything of the NEXT factor is asked for before this factor's
//       products and waits in registers.  The lanes go over the entries of T = J Sigma_m (at most 81: two passes), then over the r x r
//       entries of T J^T, symmetrised, which leave as P_m where that is asked for; with e e^T added they enter the lane's two running
//       sums, unwhitened and between R and R^T.  No thread ever holds Sigma_m (27 x 27 at most).  Plain fp64 FMAs;
//   (c) k_mn_reduce: adds the partials in a tree of fixed shape (as k_qc_reduce) in two stages -- behind every chunk one workgroup per
//       224 partials, at the end one workgroup over those sums, which writes 1/2 (T + T^T) behind them.
// fp64 only; no atomics, every sum in a fixed order, the grids a function of the factor count alone: two calls give the same bits.
#include "api_common.hpp"
#include "../../include/gpslam_hip_noise.h"

#include <cmath>
#include <numeric>

namespace impl64 {
#include "api_decl.inc"
}

namespace {

constexpr int kMnRun = 32;                      // factors per workgroup
constexpr size_t kMnSlab = (size_t)128 << 20;   // bytes of e and J a chunk may hold (slabs as sampling.hip's; four of its 32 MiB, so that a
                                                // chunk of SE(3) GPS factors is 6240 workgroups: several waves on every SIMD of the chip)
constexpr int kMnReducePer = 224;               // partials per workgroup of k_mn_reduce's first stage: 16 per run at r = 2, 3
constexpr int kMnReduceThreads = 256;

struct MnStat {
  const double *e, *J;          // the chunk's: count x ROWS, count x ROWS x (2 B + 3), by position in the order added
  const int *perm;              // the chunk's factors sorted by left state: indices into the kind's arrays
  const int *idx, *lm;          // the kind's (lm: null without landmarks)
  const double *sig, *sqi;      // the kind's base noise models: sigmas, or (not null) square-root informations
  const unsigned char *use;     // the kind's, or null: all
  int first, count;             // the chunk
  const double *S, *Sn, *Sxl, *Slm;
  int nl;
  double *part;                 // gridDim.x x 2 x ROWS x ROWS
  double *P;                    // the chunk's P_m (count x ROWS x ROWS, by position in the order added), or null
};

template <int B, int LD, int ROWS, bool TWO, bool HASLM> __global__ void __launch_bounds__(64) k_mn_stat(MnStat a) {
  static_assert(HASLM == (LD > 0), "a kind that names a landmark has its dimension");
  constexpr int BB = B * B, SB = TWO ? 2 * B : B, n = SB + LD, W3 = 2 * B + 3, RR = ROWS * ROWS;
  constexpr int NBLK = (TWO ? 3 : 1) * BB, NS = (NBLK + 63) / 64;
  constexpr int NJE = ROWS * W3 + ROWS + RR, NJ = (NJE + 63) / 64;          // [J | e | R]
  constexpr int NLM = SB * LD + LD * LD, NL = HASLM ? (NLM + 63) / 64 : 1;
  constexpr int NTE = ROWS * n, NT = (NTE + 63) / 64;
  __shared__ double Sig[n * n], Jl[NJE], T[NTE], Pl[RR];
  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * kMnRun, g1 = min(g0 + kMnRun, a.count);
  const int *perm = a.perm + a.first;
  auto next_used = [&](int g) {   // (wave-uniform)
    while (g < g1 && a.use && !a.use[perm[g]]) g++;
    return g;
  };
  double preS[NS], preJ[NJ], preL[NL];
  // everything of factor m but (blocks == false) the state blocks: consecutive lanes on consecutive doubles
  auto fetch = [&](int m, bool blocks) {
    const size_t i = (size_t)a.idx[m];
    if (blocks) {
#pragma unroll
      for (int t = 0; t < NS; t++) {
        const int q = lane + 64 * t;
        preS[t] = 0.0;
        if (q < NBLK) {
          const int blk = q / BB, e = q - blk * BB;
          const double *src = blk == 1 ? a.Sn + i * BB : a.S + (i + (blk >> 1)) * BB;
          preS[t] = src[e];
        }
      }
    }
    const size_t p = (size_t)(m - a.first);
#pragma unroll
    for (int t = 0; t < NJ; t++) {
      const int q = lane + 64 * t;
      preJ[t] = 0.0;
      if (q < ROWS * W3) preJ[t] = a.J[p * (ROWS * W3) + q];
      else if (q < ROWS * W3 + ROWS) preJ[t] = a.e[p * ROWS + (q - ROWS * W3)];
      else if (q < NJE) {
        const int k = q - ROWS * W3 - ROWS, r = k / ROWS, c = k - r * ROWS;
        if (a.sqi) preJ[t] = a.sqi[(size_t)m * RR + k];
        else if (r == c) preJ[t] = 1.0 / a.sig[(size_t)m * ROWS + r];
      }
    }
    if constexpr (HASLM) {
      const size_t l = (size_t)a.lm[m] * LD;
#pragma unroll
      for (int t = 0; t < NL; t++) {
        const int q = lane + 64 * t;
        preL[t] = 0.0;
        if (q < SB * LD) {            // rows i B .. i B + SB - 1 of Sxl (the right state's follow the left one's)
          const int r = q / LD, c = q - r * LD;
          preL[t] = a.Sxl[(i * B + r) * a.nl + l + c];
        } else if (q < NLM) {
          const int k = q - SB * LD, r = k / LD, c = k - r * LD;
          preL[t] = a.Slm[(l + r) * a.nl + l + c];
        }
      }
    }
  };
  auto jcol = [](int q) { return q < SB ? q : 2 * B + (q - SB); };   // Sigma_m's coordinate q in a row of J
  double accB = 0.0, accW = 0.0;      // lane r ROWS + s < RR: entry (r, s) of this workgroup's two partials
  int cur = -1;
  int g = next_used(g0);
  if (g < g1) fetch(perm[g], true);
  while (g < g1) {
    const int m = perm[g], i = a.idx[m];
    __syncthreads();                  // (the last factor's Sigma_m, J, T and P have been read)
    if (i != cur) {                   // Sigma_m's state part: [[S_i, Sn_i], [Sn_i^T, S_{i+1}]]
#pragma unroll
      for (int t = 0; t < NS; t++) {
        const int q = lane + 64 * t;
        if (q < NBLK) {
          const int blk = q / BB, e = q - blk * BB, r = e / B, c = e - r * B;
          if (blk == 0) Sig[r * n + c] = preS[t];
          else if (blk == 2) Sig[(B + r) * n + B + c] = preS[t];
          else { Sig[r * n + B + c] = preS[t]; Sig[(B + c) * n + r] = preS[t]; }
        }
      }
      cur = i;
    }
#pragma unroll
    for (int t = 0; t < NJ; t++) {
      const int q = lane + 64 * t;
      if (q < NJE) Jl[q] = preJ[t];
    }
    if constexpr (HASLM) {
#pragma unroll
      for (int t = 0; t < NL; t++) {
        const int q = lane + 64 * t;
        if (q < SB * LD) {
          const int r = q / LD, c = q - r * LD;
          Sig[r * n + SB + c] = preL[t];
          Sig[(SB + c) * n + r] = preL[t];
        } else if (q < NLM) {
          const int k = q - SB * LD, r = k / LD, c = k - r * LD;
          Sig[(SB + r) * n + SB + c] = preL[t];
        }
      }
    }
    __syncthreads();
    const int gn = next_used(g + 1);
    if (gn < g1) fetch(perm[gn], a.idx[perm[gn]] != cur);
    double v[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {    // T = J Sigma_m
      const int o = lane + 64 * t;
      v[t] = 0.0;
      if (o < NTE) {
        const int r = o / n, c = o - r * n;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < n; q++) s += Jl[r * W3 + jcol(q)] * Sig[q * n + c];
        v[t] = s;
      }
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {    // (T was last read before the barrier at the top)
      const int o = lane + 64 * t;
      if (o < NTE) T[o] = v[t];
    }
    __syncthreads();
    const int r = lane / ROWS, s = lane - r * ROWS;
    if (lane < RR) {
      double p = 0.0;
#pragma unroll
      for (int c = 0; c < n; c++) p += T[r * n + c] * Jl[s * W3 + jcol(c)];
      Pl[lane] = p;
    }
    __syncthreads();
    if (lane < RR) {
      const double *el = Jl + ROWS * W3, *Rl = el + ROWS;
      if (a.P) a.P[(size_t)(m - a.first) * RR + lane] = 0.5 * (Pl[r * ROWS + s] + Pl[s * ROWS + r]);
      double w = 0.0;
#pragma unroll
      for (int p = 0; p < ROWS; p++) {
        double u = 0.0;               // (U R^T)[p, s], U = 1/2 (P + P^T) + e e^T
#pragma unroll
        for (int q = 0; q < ROWS; q++) u += (0.5 * (Pl[p * ROWS + q] + Pl[q * ROWS + p]) + el[p] * el[q]) * Rl[s * ROWS + q];
        w += Rl[r * ROWS + p] * u;
      }
      accB += 0.5 * (Pl[r * ROWS + s] + Pl[s * ROWS + r]) + el[r] * el[s];
      accW += w;
    }
    g = gn;
  }
  if (lane < RR) {
    a.part[(size_t)blockIdx.x * 2 * RR + lane] = accB;
    a.part[(size_t)blockIdx.x * 2 * RR + RR + lane] = accW;
  }
}

// Workgroup g: out[g w + e] = entry e of the sum of partials g per_wg .. (g + 1) per_wg - 1 (w = 2 r r doubles each) in a tree of
// fixed shape: entry e of run t (a contiguous run of the workgroup's partials, in order) in thread t w + e, the runs in order in
// thread e.  sym (the last stage, one workgroup): both r x r matrices leave as 1/2 (T + T^T)
__global__ void __launch_bounds__(kMnReduceThreads) k_mn_reduce(const double *part, int np, int per_wg, int r, int sym, double *out) {
  __shared__ double red[kMnReduceThreads], tot[18];
  const int tid = threadIdx.x, RR = r * r, w = 2 * RR, runs = kMnReduceThreads / w;
  const int run = tid / w, e = tid - run * w;
  const int p0 = min((int)blockIdx.x * per_wg, np), p1 = min(p0 + per_wg, np), cnt = p1 - p0;
  if (run < runs) {
    const int per = (cnt + runs - 1) / runs, i0 = p0 + min(run * per, cnt), i1 = min(i0 + per, p1);
    double acc = 0.0;
    for (int i = i0; i < i1; i++) acc += part[(size_t)i * w + e];
    red[tid] = acc;
  }
  __syncthreads();
  if (tid < w) {
    double t = 0.0;
    for (int q = 0; q < runs; q++) t += red[q * w + tid];
    tot[tid] = t;
  }
  __syncthreads();
  if (tid < w) {
    const int mat = tid / RR, k = tid - mat * RR, row = k / r, col = k - row * r;
    out[(size_t)blockIdx.x * w + tid] = sym ? 0.5 * (tot[mat * RR + row * r + col] + tot[mat * RR + col * r + row]) : tot[tid];
  }
}

int mn_refuse(gpslam_hip_handle *h, int kind, const char *who) {
  const char *why = nullptr;
  if (h->cfg.precision == GPSLAM_FP32) why = "fp32 handles are not supported (fp64 only)";
  else if (sharded(h)) why = "sharded handles are not supported";
  else if (h->fs.active && h->fs.split) why = "split pieces are not supported";
  else if (h->mf == ROT3_BIAS) why = "GPSLAM_ROT3_BIAS is not supported";
  else if (kind == FK_AHRS) why = "GPSLAM_MEAS_AHRS is not supported (the factor whitens by its pre-integrated covariance itself)";
  else if (h->fs.active && h->ms[kind].haslm)
    why = "a kind that names a landmark is not supported on the segmented landmark path (S_lm and S_x_lm do not exist there)";
  if (why) return fail(h, GPSLAM_E_UNSUPPORTED, (std::string(who) + ": " + why).c_str());
  return 0;
}

template <int B, int LD, int ROWS, bool TWO> void mn_launch(gpslam_hip_handle *h, const MnStat &a, int nwg) {
  k_mn_stat<B, LD, ROWS, TWO, (LD > 0)><<<dim3(nwg), dim3(64), 0, h->stream>>>(a);
}

// the (block size, landmark dimension, rows, states) of every measurement kind on every manifold it exists for
bool mn_dispatch(gpslam_hip_handle *h, const MeasSet &s, const MnStat &a, int nwg) {
  switch (h->b * 1000 + (s.haslm ? h->ld : 0) * 100 + s.rows * 10 + (s.two ? 1 : 0)) {
    case 6211: mn_launch<6, 2, 1, true>(h, a, nwg); return true;      // interpolated range: SE(2), the 2-D linear chain
    case 12311: mn_launch<12, 3, 1, true>(h, a, nwg); return true;    //                     SE(3)
    case 6210: mn_launch<6, 2, 1, false>(h, a, nwg); return true;     // range
    case 12310: mn_launch<12, 3, 1, false>(h, a, nwg); return true;
    case 6021: mn_launch<6, 0, 2, true>(h, a, nwg); return true;      // interpolated attitude: SO(3)
    case 12031: mn_launch<12, 0, 3, true>(h, a, nwg); return true;    // interpolated GPS: SE(3)
    case 6031: mn_launch<6, 0, 3, true>(h, a, nwg); return true;      // odometry: the 2-D linear chain
    case 6220: mn_launch<6, 2, 2, false>(h, a, nwg); return true;     // bearing-range
    case 12321: mn_launch<12, 3, 2, true>(h, a, nwg); return true;    // interpolated projection: SE(3)
  }
  return false;
}

// the statistic (out18: [B | Bw], or null) or the predicted covariances (P, or null) of one kind
int mn_run(gpslam_hip_handle *h, int kind, const uint8_t *use, double *out18, double *P, const char *who) {
  MeasSet &s = h->ms[kind];
  const int F = s.count(), rows = s.rows, RR = rows * rows, W3 = 2 * h->b + 3;
  (void)hipSetDevice(h->cfg.device);
  int per = (int)(kMnSlab / ((size_t)rows * (W3 + 1) * sizeof(double))) / kMnRun * kMnRun;
  per = std::min(per, F);
  const int nchunks = nblocks(F, per);
  MeasNoise &mn = h->mn;
  mn.fit(h->N);
  if (!mn.have[kind]) {             // a stable sort by left state inside every chunk
    std::vector<int> perm((size_t)F);
    std::iota(perm.begin(), perm.end(), 0);
    for (int c = 0; c < nchunks; c++)
      std::stable_sort(perm.begin() + (size_t)c * per, perm.begin() + std::min((size_t)F, ((size_t)c + 1) * per),
                       [&](int x, int y) { return s.idx[x] < s.idx[y]; });
    HIPCHK(upload_vec(h->stream, mn.perm[kind], perm));
    mn.have[kind] = true;
  }
  if (use) {
    HIPCHK(mn.use.reserve((size_t)F));
    HIPCHK(hipMemcpyAsync(mn.use.p, use, (size_t)F, hipMemcpyHostToDevice, h->stream));
  }
  const int maxwg = nblocks(per, kMnRun);
  size_t stage2 = 0;                // the first stage's sums of every chunk, in chunk order
  for (int c = 0; c < nchunks; c++) stage2 += (size_t)nblocks(nblocks(std::min(per, F - c * per), kMnRun), kMnReducePer);
  HIPCHK(h->api_e.reserve((size_t)per * rows * sizeof(double)));
  HIPCHK(h->api_H.reserve((size_t)per * rows * W3 * sizeof(double)));
  HIPCHK(mn.part.reserve((size_t)maxwg * 2 * RR * sizeof(double)));
  HIPCHK(mn.cpart.reserve((stage2 + 1) * 2 * RR * sizeof(double)));       // (the result behind them)
  if (P) HIPCHK(mn.P.reserve((size_t)per * RR * sizeof(double)));
  MnStat a;
  a.e = h->api_e.as<double>(); a.J = h->api_H.as<double>();
  a.perm = mn.perm[kind].as<int>(); a.idx = s.d_idx.as<int>(); a.lm = s.haslm ? s.d_lm.as<int>() : nullptr;
  a.sig = s.d_sig.as<double>(); a.sqi = s.sqi.empty() ? nullptr : s.d_sqi.as<double>();
  a.use = use ? mn.use.as<unsigned char>() : nullptr;
  a.S = h->mg.S.as<double>(); a.Sn = h->mg.Sn.as<double>(); a.Sxl = h->mg.Sxl.as<double>(); a.Slm = h->mg.Slm.as<double>();
  a.nl = h->nl; a.part = mn.part.as<double>(); a.P = P ? mn.P.as<double>() : nullptr;
  double *cpart = mn.cpart.as<double>();
  size_t done = 0;
  for (int c = 0; c < nchunks; c++) {
    a.first = c * per; a.count = std::min(per, F - a.first);
    int rc = impl64::launch_meas_inspect(h, kind, a.first, a.count, h->api_e.p, h->api_H.p);
    if (rc) return rc;
    const int nwg = nblocks(a.count, kMnRun), nred = nblocks(nwg, kMnReducePer);
    if (!mn_dispatch(h, s, a, nwg)) return fail(h, GPSLAM_E_UNSUPPORTED, (std::string(who) + ": no kernel for this kind on this manifold").c_str());
    if (out18) k_mn_reduce<<<dim3(nred), dim3(kMnReduceThreads), 0, h->stream>>>(a.part, nwg, kMnReducePer, rows, 0, cpart + done * 2 * RR);
    done += nred;
    HIPCHK(hipGetLastError());
    if (P) HIPCHK(hipMemcpyAsync(P + (size_t)a.first * RR, mn.P.p, (size_t)a.count * RR * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  if (out18) {
    double *res = cpart + stage2 * 2 * RR;
    k_mn_reduce<<<dim3(1), dim3(kMnReduceThreads), 0, h->stream>>>(cpart, (int)stage2, (int)stage2, rows, 1, res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out18, res, 2 * RR * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

bool mn_finite(int r, const double *M) {
  for (int i = 0; i < r * r; i++)
    if (!std::isfinite(M[i])) return false;
  return true;
}
bool mn_sym_spd(int r, const double *M) {
  double C[9];
  if (!mn_finite(r, M)) return false;
  for (int i = 0; i < r; i++)
    for (int j = 0; j < r; j++) C[i * r + j] = 0.5 * (M[i * r + j] + M[j * r + i]);
  return spd_chol_upper(r, C);
}

}  // namespace

extern "C" {

int gpslam_hip_meas_noise_statistic(gpslam_hip_handle *h, int32_t kind, const uint8_t *use, double *B, double *Bw, int64_t *n) {
  if (!h || kind < 0 || kind >= kNumMeasKinds) return GPSLAM_E_INVALID;
  int rc;
  if ((rc = mn_refuse(h, kind, "meas_noise_statistic")) || (rc = marginals_getter_check(h))) return rc;
  const MeasSet &s = h->ms[kind];
  const int F = s.count(), RR = s.rows * s.rows;
  int64_t used = 0;
  for (int f = 0; f < F; f++) {
    if (use && !use[f]) continue;
    used++;
    if (!s.rob.empty() && s.rob[2 * (size_t)f] != 0.0)
      return fail(h, GPSLAM_E_UNSUPPORTED, "meas_noise_statistic: a used factor carries a robust loss (the Gaussian M-step does not apply to it; leave it out with `use`)");
  }
  if (n) *n = used;
  if (B) for (int i = 0; i < RR; i++) B[i] = 0.0;
  if (Bw) for (int i = 0; i < RR; i++) Bw[i] = 0.0;
  if (used == 0 || (!B && !Bw)) return 0;
  double out[18];
  if ((rc = mn_run(h, kind, use, out, nullptr, "meas_noise_statistic"))) return rc;
  if (B) for (int i = 0; i < RR; i++) B[i] = out[i];
  if (Bw) for (int i = 0; i < RR; i++) Bw[i] = out[RR + i];
  return 0;
}

int gpslam_hip_meas_predicted_covariances(gpslam_hip_handle *h, int32_t kind, double *P) {
  if (!h || kind < 0 || kind >= kNumMeasKinds) return GPSLAM_E_INVALID;
  int rc;
  if ((rc = mn_refuse(h, kind, "meas_predicted_covariances"))) return rc;
  const int F = h->ms[kind].count();
  if (F == 0 || !P) return F;       // (P == NULL: the count alone, from the stored graph)
  if ((rc = marginals_getter_check(h))) return rc;
  if ((rc = mn_run(h, kind, nullptr, nullptr, P, "meas_predicted_covariances"))) return rc;
  return F;
}

int gpslam_hip_noise_gradient(int32_t r, const double *C, const double *B, int64_t n, double *G) {
  if (r < 1 || r > 3 || !C || !B || !G || n <= 0 || !mn_sym_spd(r, C) || !mn_finite(r, B)) return GPSLAM_E_INVALID;
  for (int i = 0; i < r * r; i++) G[i] = 0.5 * ((double)n * C[i] - B[i]);
  return 0;
}

int gpslam_hip_noise_em_update(int32_t r, const double *B, int64_t n, double *C_next) {
  if (r < 1 || r > 3 || !B || !C_next || n <= 0 || !mn_sym_spd(r, B)) return GPSLAM_E_INVALID;
  const double s = 1.0 / (double)n;
  for (int i = 0; i < r; i++)
    for (int j = 0; j < r; j++) C_next[i * r + j] = 0.5 * (B[i * r + j] + B[j * r + i]) * s;
  return 0;
}

int gpslam_hip_noise_em_scale(int32_t r, const double *Bw, int64_t n, double *ratio, double *ratio_rows) {
  if (r < 1 || r > 3 || !Bw || !ratio || n <= 0 || !mn_sym_spd(r, Bw)) return GPSLAM_E_INVALID;
  double tr = 0.0;
  for (int q = 0; q < r; q++) {
    tr += Bw[q * r + q];
    if (ratio_rows) ratio_rows[q] = Bw[q * r + q] / (double)n;
  }
  *ratio = tr / ((double)n * (double)r);
  return 0;
}

}  // extern "C"
