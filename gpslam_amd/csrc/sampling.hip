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
#include "api_common.hpp"
#include "../../include/gpslam_hip_sampling.h"

#include <cmath>

namespace impl64 {
#include "api_decl.inc"
}

namespace {

// doubles per staging / output slab at most (32 MiB): a chunk of draws is as many as fit, at least one
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

// draws per chunk: the widest slab row decides
int ps_chunk(const gpslam_hip_handle *h, int count) {
  const size_t widest = std::max<size_t>({(size_t)ps_noise_dim(h), (size_t)h->N * h->b + (size_t)h->nl, (size_t)h->N * h->pd, 1});
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

// the draws, chunk by chunk, over the linearisation in place
int ps_draws(gpslam_hip_handle *h, const LaunchMode &m, int count, uint64_t seed, uint64_t first, const double *noise, const PsOut &o) {
  int rc;
  const int N = h->N, b = h->b, nl = h->nl, n_noise = ps_noise_dim(h), chunk = ps_chunk(h, count);
  const size_t wd = (size_t)N * b + nl, wp = (size_t)N * h->pd, wv = (size_t)N * h->d;
  HIPCHK(h->ps.stage.reserve(std::max<size_t>((size_t)chunk * n_noise, 1) * sizeof(double)));
  if (o.delta) HIPCHK(h->ps.delta.reserve((size_t)chunk * wd * sizeof(double)));
  if (o.poses) HIPCHK(h->ps.poses.reserve((size_t)chunk * wp * sizeof(double)));
  if (o.vels) HIPCHK(h->ps.vels.reserve((size_t)chunk * wv * sizeof(double)));
  if (o.lms && nl > 0) HIPCHK(h->ps.lms.reserve((size_t)chunk * nl * sizeof(double)));
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
  for (int k0 = 0; k0 < count; k0 += chunk) {
    const int nk = std::min(chunk, count - k0);
    double *stage = h->ps.stage.as<double>();
    if (noise) {
      if (n_noise > 0) HIPCHK(hipMemcpyAsync(stage, noise + (size_t)k0 * n_noise, (size_t)nk * n_noise * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else if (n_noise > 0 && (rc = ps_generate(h, seed, first + (uint64_t)k0, nk, n_noise, stage))) return rc;
    for (int k = 0; k < nk; k++) {
      pa.eps = stage + (size_t)k * n_noise;
      if (n_noise > 0) k_ps_place<<<dim3(nblocks(n_noise, 256)), dim3(256), 0, h->stream>>>(pa);
      if ((rc = impl64::launch_assemble(h, m, false)) || (rc = impl64::launch_solve(h, m, 0.0))) return rc;
      ea.delta = o.delta ? h->ps.delta.as<double>() + (size_t)k * wd : nullptr;
      ea.poses = o.poses ? h->ps.poses.as<double>() + (size_t)k * wp : nullptr;
      ea.vels = o.vels ? h->ps.vels.as<double>() + (size_t)k * wv : nullptr;
      ea.lms = (o.lms && nl > 0) ? h->ps.lms.as<double>() + (size_t)k * nl : nullptr;
      dispatch_mf(h->mf, [&](auto tag) { k_ps_emit<decltype(tag)::value><<<dim3(nblocks(N + nl, 128)), dim3(128), 0, h->stream>>>(ea); });
      HIPCHK(hipGetLastError());
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
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int ps_sample(gpslam_hip_handle *h, int count, uint64_t seed, uint64_t first, const double *noise, const PsOut &o) {
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
    rc = ps_draws(h, m, count, seed, first, noise, o);
  }
  // the linearisation's own errors back into the tables: the handle is as a call of gpslam_hip_get_rows leaves it
  if (nE) HIPCHK(hipMemcpyAsync(h->rowE.p, save, nE, hipMemcpyDeviceToDevice, h->stream));
  if (nCE) HIPCHK(hipMemcpyAsync(h->rowCE.p, save + nE, nCE, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return rc;
}

}  // namespace

extern "C" {

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
  const int n_noise = ps_noise_dim(h);
  if (n_noise == 0) return 0;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)count, kPsSlab / (size_t)n_noise));
  HIPCHK(h->ps.stage.reserve((size_t)chunk * n_noise * sizeof(double)));
  for (int k0 = 0; k0 < count; k0 += chunk) {
    const int nk = std::min(chunk, count - k0);
    if ((rc = ps_generate(h, seed, first + (uint64_t)k0, nk, n_noise, h->ps.stage.as<double>()))) return rc;
    HIPCHK(hipMemcpyAsync(noise + (size_t)k0 * n_noise, h->ps.stage.p, (size_t)nk * n_noise * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int gpslam_hip_sample_posterior(gpslam_hip_handle *h, int32_t count, uint64_t seed, uint64_t first,
                                const double *noise, double *delta, double *poses, double *vels, double *landmarks) {
  if (!h || count <= 0 || (!delta && !poses && !vels && !landmarks)) return GPSLAM_E_INVALID;
  int rc = ps_guard(h, "sample_posterior");
  if (rc) return rc;
  return ps_sample(h, count, seed, first, noise, PsOut{delta, poses, vels, landmarks});
}

}  // extern "C"
