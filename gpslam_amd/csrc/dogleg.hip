// dogleg.hip -- Powell's dogleg optimiser (gtsam::DoglegOptimizer; include/gpslam_hip_dogleg.h): one linearisation and ONE solve per
// iteration, every trial of a trust radius a blend of two vectors that are already on the device, a retraction and an error pass.
// fp64, unsharded handles with the dense landmark border (or none); DESIGN.md section 4i has the algebra and the launch sequence.
//
// Per iteration: the linearisation (rows, error, records [D | O | g | B] with the gradient copied to gsave) -> k_dl_lm (landmarks: g_L
// and its share of g^T H g, g . g) -> k_dl_quad (the records' share, before the elimination overwrites them) -> one fixed-order sum
// -> launch_solve (lambda = 0) -> the Gauss-Newton step kept (dvec, dl.nL) -> g . dn, dn . dn -> ONE read of the scalars.  Per
// trial: gpslam_hip_dogleg_point on the host -> k_dl_blend writes alpha g + beta dn where the retraction reads it -> launch_retract
// and an error pass -> gpslam_hip_dogleg_decide on the host.
#include "api_common.hpp"
#include "../../include/gpslam_hip_dogleg.h"

#include <cmath>

namespace impl64 {
#include "api_decl.inc"
}

namespace {

typedef double DlV2 __attribute__((ext_vector_type(2)));

constexpr int kDlStates = 8;    // states per wave: a contiguous run, its gradients staged once in LDS
constexpr int kDlWaves = 4;     // waves per workgroup
constexpr int kDlBorder = kMaxRhs - 1;   // landmark coordinates of the dense border at most

struct DlQuadArgs {
  const double *blk;      // N records [D | O | R right-hand-side columns], column 0 = g, columns 1 .. nl = B
  const double *g;        // N x B: the gradient (gsave)
  const double *gL;       // nl: the landmark gradient (k_dl_lm) or null
  int N, R, nl;
  double *part;           // [g^T H g: nb_total | g . g: nb_total]; this kernel's workgroups come first
  int nb_total;
};

// g^T H g and g . g over the records, one pass.  A wave owns kDlStates consecutive states: it stages their gradients, the next
// state's and g_L in LDS, then streams the records -- lane l takes the 16-byte pairs l, l + 64, ... of every record, so a wave's load
// instruction covers 1 KiB of consecutive addresses.  What an element of the record multiplies does not depend on the state: lane
// and slot fix (row, column) once, in front of the loop (`meta`).  Per state
//     g_i^T D_i g_i + 2 g_{i+1}^T O_i g_i + 2 g_i^T B_i g_L          (O_i = H_{i+1,i}, row-major: k_assemble_ghost stores lane c's
//                                                                     sums of R_c L_k at [B * B + c * B + k])
// and g_i . g_i from the record's own gradient column.  Two states are in flight per wave (two register sets, no copies).  Sums: lane,
// wave (shuffle tree), workgroup (four waves in order) -> part; a second launch adds the workgroups' numbers in fixed order.
// 16-byte pairs per lane and record: of a chain without landmarks (R = 1), and at most (R = kMaxRhs)
constexpr int dl_slots(int B, int R) { return (2 * B * B + B * R + 127) / 128; }
// MAXS: the slots the instantiation holds registers for -- dl_slots(B, 1) for records without landmark columns (B = 12: 3 slots, not
// 5), dl_slots(B, kMaxRhs) otherwise; `nslot` (wave-uniform) skips the loads and the arithmetic of slots a narrower record leaves empty
template <int B, int MAXS>
__global__ void __launch_bounds__(64 * kDlWaves) k_dl_quad(DlQuadArgs a) {
  constexpr int S = kDlStates;
  constexpr int GL0 = (S + 1) * B;                                // g_L behind the states' gradients
  __shared__ double gs[kDlWaves][GL0 + kDlBorder + 1];
  __shared__ double red[2][kDlWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s0 = (blockIdx.x * kDlWaves + w) * S;
  const int ns = min(S, a.N - s0);                                // (<= 0: a wave behind the chain's end)
  const int BS = 2 * B * B + B * a.R, npair = BS / 2, nslot = (npair + 63) / 64;     // (nslot <= MAXS: the launcher's choice)
  double *gw = gs[w];
  for (int i = lane; i < GL0; i += 64) gw[i] = (s0 + i / B < a.N) ? a.g[(size_t)s0 * B + i] : 0.0;   // zeros behind the last state
  for (int i = lane; i <= kDlBorder; i += 64) gw[GL0 + i] = (i < a.nl) ? a.gL[i] : 0.0;
  wave_lds_sync();
  // element e of a record: bits 0-7 index of the first gradient factor (relative to the state's), 8-15 of the second, 16: the second
  // is relative to the state's too (not g_L), 17-18 the weight (0, 1, 2), 19: the element is the gradient itself (g . g)
  int meta[MAXS][2];
#pragma unroll
  for (int t = 0; t < MAXS; t++)
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int e = 2 * (t * 64 + lane) + u;
      int m = 0;
      if (e < B * B) m = (e / B) | ((e % B) << 8) | (1 << 16) | (1 << 17);
      else if (e < 2 * B * B) m = (B + (e - B * B) / B) | (((e - B * B) % B) << 8) | (1 << 16) | (2 << 17);
      else if (e < BS) {
        const int r = (e - 2 * B * B) / B, k = (e - 2 * B * B) % B;
        if (r == 0) m = 1 << 19;
        else if (r <= a.nl) m = k | ((GL0 + r - 1) << 8) | (2 << 17);
      }
      meta[t][u] = m;
    }
  auto ldst = [&](int j, DlV2 (&v)[MAXS]) {
    const double *rec = a.blk + (size_t)(s0 + j) * BS;
#pragma unroll
    for (int t = 0; t < MAXS; t++) {
      const int q = t * 64 + lane;
      if (t < nslot) v[t] = *reinterpret_cast<const DlV2 *>(rec + 2 * (q < npair ? q : 0));   // (clamped, not predicated; meta is 0 there)
    }
  };
  double acc = 0.0, accg = 0.0;
  auto use = [&](int j, const DlV2 (&v)[MAXS]) {
    const int base = j * B;
#pragma unroll
    for (int t = 0; t < MAXS; t++)
#pragma unroll
      for (int u = 0; u < 2; u++) {
        if (t >= nslot) continue;
        const int m = meta[t][u];
        const double val = u == 0 ? v[t].x : v[t].y;
        const double xa = gw[base + (m & 0xff)];
        const double xb = gw[((m >> 8) & 0xff) + (((m >> 16) & 1) ? base : 0)];
        const double wq = (double)((m >> 17) & 3);
        acc += wq * (xa * val * xb);
        if ((m >> 19) & 1) accg += val * val;
      }
  };
  DlV2 va[MAXS], vb[MAXS];
  if (ns > 0) ldst(0, va);
  for (int j = 0; j < ns; j += 2) {
    if (j + 1 < ns) ldst(j + 1, vb);
    use(j, va);
    if (j + 2 < ns) ldst(j + 2, va);
    if (j + 1 < ns) use(j + 1, vb);
  }
  acc = wave_sum(acc);
  accg = wave_sum(accg);
  if (lane == 0) { red[0][w] = acc; red[1][w] = accg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0, sg = 0.0;
    for (int i = 0; i < kDlWaves; i++) { s += red[0][i]; sg += red[1][i]; }
    a.part[blockIdx.x] = s;
    a.part[a.nb_total + blockIdx.x] = sg;
  }
}

struct DlLmArgs {
  const double *rowE, *rowM;        // the row tables: whitened error, landmark columns (M x ld)
  const int *lmrow, *lmrow_ptr;     // rows that name a landmark, grouped by landmark
  int ld, L;
  int npri;                         // landmark priors
  const int *pri_lm;
  const double *pri_meas, *pri_sig, *lmk;
  double *gL;                       // out: L x ld
  double *part;                     // [g^T H g | g . g]: this kernel's L numbers sit behind k_dl_quad's nbq
  int nbq, nb_total;
};

// One workgroup per landmark.  First its gradient g_L = -sum_rows rowM e (+ the priors'), the sums k_lm_reduce_part forms for the
// Schur complement's right-hand side; then, with g_L known, its share of g^T H g: H_LL is block diagonal over the landmarks (a row
// names one), so g_L^T H_LL g_L = sum_rows (rowM . g_L)^2 + sum_priors (g_L,q / sigma_q)^2.  Fixed order: thread, wave, workgroup.
__global__ void __launch_bounds__(256) k_dl_lm(DlLmArgs a) {
  __shared__ double red[3][4];
  __shared__ double gsh[3];
  const int lm = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j0 = a.lmrow_ptr[lm], j1 = a.lmrow_ptr[lm + 1];
  double g[3] = {0.0, 0.0, 0.0};
  for (int j = j0 + (int)threadIdx.x; j < j1; j += 256) {
    const int rho = a.lmrow[j];
    const double e = a.rowE[rho];
    for (int q = 0; q < a.ld; q++) g[q] -= a.rowM[(size_t)rho * a.ld + q] * e;
  }
  for (int q = 0; q < 3; q++) {
    const double v = wave_sum(g[q]);
    if (lane == 0) red[q][w] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 0; q < a.ld; q++) {
      double s = 0.0;
      for (int i = 0; i < 4; i++) s += red[q][i];
      for (int k = 0; k < a.npri; k++) {
        if (a.pri_lm[k] != lm) continue;
        const double wk = 1.0 / a.pri_sig[(size_t)k * a.ld + q];
        s -= wk * wk * (a.lmk[(size_t)lm * a.ld + q] - a.pri_meas[(size_t)k * a.ld + q]);
      }
      gsh[q] = s;
      a.gL[(size_t)lm * a.ld + q] = s;
    }
  }
  __syncthreads();
  double acc = 0.0;
  for (int j = j0 + (int)threadIdx.x; j < j1; j += 256) {
    const int rho = a.lmrow[j];
    double t = 0.0;
    for (int q = 0; q < a.ld; q++) t += a.rowM[(size_t)rho * a.ld + q] * gsh[q];
    acc += t * t;
  }
  acc = wave_sum(acc);
  if (lane == 0) red[0][w] = acc;     // (red[0] was read by thread 0 alone, in front of the barrier above)
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0, sg = 0.0;
    for (int i = 0; i < 4; i++) s += red[0][i];
    for (int k = 0; k < a.npri; k++) {
      if (a.pri_lm[k] != lm) continue;
      for (int q = 0; q < a.ld; q++) {
        const double t = gsh[q] / a.pri_sig[(size_t)k * a.ld + q];
        s += t * t;
      }
    }
    for (int q = 0; q < a.ld; q++) sg += gsh[q] * gsh[q];
    a.part[a.nbq + lm] = s;
    a.part[a.nb_total + a.nbq + lm] = sg;
  }
}

struct DlBlendArgs {
  const double *g, *dn;     // N x B: gradient (gsave), Gauss-Newton step (dvec)
  const double *gL, *nL;    // nl: the same of the landmarks
  double *x;                // level-0 solution array, N x R x B: column 0 is what the retraction reads
  double *dL;               // nl: lm_dL
  int N, B, R, nl;
  int pad0;                 // coordinates pad0 .. B - 1 of a block are pads (GPSLAM_ROT3_BIAS: 9), or B
  double alpha, beta;
};
// delta_d = alpha g + beta delta_n into column 0 of the level-0 solution and into lm_dL; pads get an exact 0
__global__ void __launch_bounds__(256) k_dl_blend(DlBlendArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nx = a.N * a.B;
  if (i < nx) {
    const int s = i / a.B, k = i - s * a.B;
    const double v = a.alpha * a.g[i] + a.beta * a.dn[i];
    a.x[(size_t)s * a.R * a.B + k] = (k >= a.pad0) ? 0.0 : v;
  } else if (i < nx + a.nl) {
    const int j = i - nx;
    a.dL[j] = a.alpha * a.gL[j] + a.beta * a.nL[j];
  }
}

bool dl_mode_ok(int32_t mode) { return mode >= GPSLAM_DOGLEG_ONE_STEP_PER_ITERATION && mode <= GPSLAM_DOGLEG_SEARCH_REDUCE_ONLY; }

// every refusal, before anything is launched
int dl_guard(gpslam_hip_handle *h, const char *what) {
  int rc = need_compiled(h);
  if (rc) return rc;
  const char *why = nullptr;
  if (h->cfg.precision != GPSLAM_FP64) why = "an fp32 handle (the dogleg's quadratic form and blend are fp64 kernels)";
  else if (h->fs.active && h->fs.split) why = "a piece of a split chain";
  else if (sharded(h)) why = "a sharded handle";
  else if (h->fs.active) why = "the segmented landmark path (the records carry no landmark columns there)";
  else if (h->clo.n > 0) why = "loop closures (their blocks and gradient are not in the records)";
  else if (h->bg.count() > 0) why = "border Gaussians (their landmark block is not in the row tables)";
  if (why) return fail(h, GPSLAM_E_UNSUPPORTED, (std::string(what) + ": not supported on " + why).c_str());
  (void)hipSetDevice(h->cfg.device);
  return 0;
}

// scal slots: 0 error at the linearisation point, 1 trial error, 2 |delta|_inf (the launch helpers'); 3 g . dn and 4 dn . dn over the
// states, 5 and 6 over the landmarks; 9 g^T H g, 10 g . g
enum { DL_GN_X = 3, DL_NN_X = 4, DL_GN_L = 5, DL_NN_L = 6, DL_GHG = 9, DL_GG = 10 };

// linearise, the four scalars, the one solve: s4 = {gg, gHg, gn, nn}, *f the error at the linearisation point
int dl_prepare(gpslam_hip_handle *h, double *s4, double *f) {
  int rc;
  const int N = h->N, b = h->b, R = h->R, nl = h->nl, nx = N * b;
  const int nbq = nblocks(N, kDlStates * kDlWaves), nbt = nbq + (nl > 0 ? h->L : 0), nbd = nblocks(nx, 256);
  // [quadratic form: 2 nbt | dots over the states: 3 nbd | dots over the landmarks: 3]
  HIPCHK(h->dl.part.reserve(((size_t)2 * nbt + 3 * (size_t)nbd + 3) * sizeof(double)));
  HIPCHK(h->dl.gL.reserve((size_t)std::max(nl, 1) * sizeof(double)));
  HIPCHK(h->dl.nL.reserve((size_t)std::max(nl, 1) * sizeof(double)));
  double *part = h->dl.part.as<double>(), *pdx = part + 2 * (size_t)nbt, *pdl = pdx + 3 * (size_t)nbd;
  double *scal = h->scal.as<double>();
  // the pivot flag cleared; rows and the error of the current estimate (scal[0]); the estimate remembered; the records [D | O | g | B]
  // in the form of gpslam_hip_normal_equations, the gradient copied to gsave
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  if ((rc = impl64::launch_factors(h, LaunchMode{}, 0, 0)) || (rc = backup_state(h, false)) || (rc = impl64::launch_assemble(h, LaunchMode{}, true))) return rc;
  if (nl > 0) {
    DlLmArgs la;
    la.rowE = h->rowE.as<double>(); la.rowM = h->rowM.as<double>();
    la.lmrow = h->lmrow.as<int>(); la.lmrow_ptr = h->lmrow_ptr.as<int>();
    la.ld = h->ld; la.L = h->L;
    la.npri = h->lpri.count(); la.pri_lm = h->lpri.d_idx.as<int>(); la.pri_meas = h->lpri.d_meas.as<double>(); la.pri_sig = h->lpri.d_sig.as<double>();
    la.lmk = h->lmk.as<double>(); la.gL = h->dl.gL.as<double>(); la.part = part; la.nbq = nbq; la.nb_total = nbt;
    k_dl_lm<<<dim3(h->L), dim3(256), 0, h->stream>>>(la);
  }
  DlQuadArgs qa;
  qa.blk = h->lv[0].blk.as<double>(); qa.g = h->gsave.as<double>(); qa.gL = nl > 0 ? h->dl.gL.as<double>() : nullptr;
  qa.N = N; qa.R = R; qa.nl = nl; qa.part = part; qa.nb_total = nbt;
  dispatch_b(b, [&](auto tag) {
    constexpr int BB = decltype(tag)::value;
    if (R == 1) k_dl_quad<BB, dl_slots(BB, 1)><<<dim3(nbq), dim3(64 * kDlWaves), 0, h->stream>>>(qa);
    else k_dl_quad<BB, dl_slots(BB, kMaxRhs)><<<dim3(nbq), dim3(64 * kDlWaves), 0, h->stream>>>(qa);
  });
  k_final_reduce3<double><<<dim3(2), dim3(256), 0, h->stream>>>(part, nbt, scal, DL_GHG, DL_GG, -1);
  HIPCHK(hipGetLastError());
  if ((rc = impl64::launch_solve(h, LaunchMode{}, 0.0))) return rc;   // (lambda = 0, level 0 unfused: the two-launch form)
  // the Gauss-Newton step is kept: the trials overwrite column 0 of the level-0 solution and lm_dL
  double *dv = h->dvec.as<double>();
  k_gather_delta<double><<<dim3(nblocks(nx, 256)), dim3(256), 0, h->stream>>>(h->lv[0].x.as<double>(), N, R, b, dv);
  k_dot3<double><<<dim3(nbd), dim3(256), 0, h->stream>>>(dv, h->gsave.as<double>(), nullptr, nx, pdx);
  k_final_reduce3<double><<<dim3(3), dim3(256), 0, h->stream>>>(pdx, nbd, scal, DL_GN_X, -1, DL_NN_X);
  if (nl > 0) {
    HIPCHK(hipMemcpyAsync(h->dl.nL.p, h->lm_dL.p, (size_t)nl * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    k_dot3<double><<<dim3(1), dim3(256), 0, h->stream>>>(h->dl.nL.as<double>(), h->dl.gL.as<double>(), nullptr, nl, pdl);
    k_final_reduce3<double><<<dim3(3), dim3(256), 0, h->stream>>>(pdl, 1, scal, DL_GN_L, -1, DL_NN_L);
  }
  HIPCHK(hipGetLastError());
  double s[11];
  int flag = 0;
  if ((rc = read_scal(h, s, 11, &flag))) return rc;
  if (flag) return fail(h, GPSLAM_E_NOT_SPD, "non-positive pivot in the block elimination");
  *f = s[0];
  s4[0] = s[DL_GG]; s4[1] = s[DL_GHG];
  s4[2] = s[DL_GN_X] + (nl > 0 ? s[DL_GN_L] : 0.0);
  s4[3] = s[DL_NN_X] + (nl > 0 ? s[DL_NN_L] : 0.0);
  return 0;
}

int dl_blend(gpslam_hip_handle *h, double alpha, double beta) {
  DlBlendArgs a;
  a.g = h->gsave.as<double>(); a.dn = h->dvec.as<double>(); a.gL = h->dl.gL.as<double>(); a.nL = h->dl.nL.as<double>();
  a.x = h->lv[0].x.as<double>(); a.dL = h->lm_dL.as<double>();
  a.N = h->N; a.B = h->b; a.R = h->R; a.nl = h->nl;
  a.pad0 = h->mf == ROT3_BIAS ? 9 : h->b;
  a.alpha = alpha; a.beta = beta;
  k_dl_blend<<<dim3(nblocks(h->N * h->b + h->nl, 256)), dim3(256), 0, h->stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}

int dl_iterate(gpslam_hip_handle *h, double *delta, int32_t mode, gpslam_hip_stats *st) {
  int rc;
  double s4[4], f = 0.0;
  if ((rc = dl_prepare(h, s4, &f))) return rc;
  if (!(f == f)) return fail(h, GPSLAM_E_NAN, "NaN error at the linearisation point");
  double coef[2] = {0, 0}, norm = 0.0, pred = 0.0, f_new = f, dinf = 0.0;
  int32_t branch = 2, last_action = 0, keep = 0, stay = 1;
  int trials = 0;
  bool moved = false;                        // the states are a trial's, not the linearisation point's
  while (stay) {
    if ((rc = ::gpslam_hip_dogleg_point(s4, *delta, coef, &norm, &pred, &branch))) return rc;
    if (moved && (rc = backup_state(h, true))) return rc;
    if ((rc = dl_blend(h, coef[0], coef[1]))) return rc;
    // the tail of a Levenberg-Marquardt trial: retract by column 0 of the level-0 solution and lm_dL (scal[2] = |delta|_inf), error into scal[1]
    if ((rc = impl64::launch_retract(h, LaunchMode{}, 2)) || (rc = impl64::launch_factors(h, LaunchMode{}, 1, 1))) return rc;
    moved = true;
    double s[3];
    int flag = 0;
    if ((rc = read_scal(h, s, 3, &flag))) return rc;
    f_new = s[1]; dinf = s[2];
    trials++;
    const double d4[4] = {f, f_new, pred, norm};
    if ((rc = ::gpslam_hip_dogleg_decide(d4, mode, delta, &last_action, &keep, &stay))) return rc;
  }
  // (the one deviation from GTSAM: a loop that ends on an increase of the cost keeps nothing)
  const bool accepted = keep && !(f_new > f) && f_new == f_new;
  if (!accepted && (rc = backup_state(h, true))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < 4; i++) h->dl.last[i] = s4[i];
  h->dl.last[4] = coef[0]; h->dl.last[5] = coef[1]; h->dl.last[6] = pred; h->dl.last[7] = (double)branch;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->error_before = f; st->error_after = accepted ? f_new : f; st->delta_inf_norm = accepted ? dinf : 0.0;
    st->lambda = *delta; st->iterations = 1; st->accepted = accepted ? 1 : 0; st->trials = trials; st->last_trial_error = f_new;
  }
  return 0;
}

}  // namespace

extern "C" {

int gpslam_hip_dogleg_point(const double *s4, double delta, double *coef2, double *step_norm, double *predicted, int32_t *branch) {
  if (!s4 || !coef2 || !(delta > 0.0) || !std::isfinite(delta)) return GPSLAM_E_INVALID;
  const double gg = s4[0], gHg = s4[1], gn = s4[2], nn = s4[3];
  const double norm_n = nn > 0.0 ? std::sqrt(nn) : 0.0;
  double alpha = 0.0, beta = 0.0;
  int32_t br = 2;
  if (!(gg > 0.0) || !(gHg > 0.0)) {            // no Cauchy point: the Gauss-Newton step, clipped to the trust region
    beta = norm_n > 0.0 ? std::fmin(1.0, delta / norm_n) : 0.0;
  } else {
    const double s = gg / gHg, uu = s * s * gg, norm_u = std::sqrt(uu);
    if (delta < norm_u) {
      alpha = delta / std::sqrt(gg);           // (Delta / |du|) s
      br = 0;
    } else if (delta < norm_n) {                // ComputeBlend: |du + tau (dn - du)| = Delta, the root in [0, 1]
      const double un = s * gn;
      const double a = uu - 2.0 * un + nn, b = 2.0 * (un - uu), c = uu - delta * delta;   // c <= 0 <= a
      double tau = 1.0;
      if (a > 0.0) {
        const double disc = std::sqrt(std::fmax(b * b - 4.0 * a * c, 0.0));
        tau = b >= 0.0 ? (-2.0 * c) / (b + disc) : (-b + disc) / (2.0 * a);               // (no cancellation in either form)
        tau = std::fmin(1.0, std::fmax(0.0, tau));
      }
      alpha = (1.0 - tau) * s;
      beta = tau;
      br = 1;
    } else {
      beta = 1.0;
    }
  }
  coef2[0] = alpha; coef2[1] = beta;
  if (step_norm) *step_norm = std::sqrt(std::fmax(alpha * alpha * gg + 2.0 * alpha * beta * gn + beta * beta * nn, 0.0));
  if (predicted) *predicted = (alpha * gg + beta * gn) - 0.5 * (alpha * alpha * gHg + 2.0 * alpha * beta * gg + beta * beta * gn);
  if (branch) *branch = br;
  return 0;
}

int gpslam_hip_dogleg_decide(const double *s4, int32_t mode, double *delta, int32_t *last_action, int32_t *keep, int32_t *stay) {
  if (!s4 || !delta || !last_action || !keep || !stay || !dl_mode_ok(mode)) return GPSLAM_E_INVALID;
  const double f = s4[0], f_new = s4[1], pred = s4[2], norm = s4[3];
  constexpr double kFloor = 1e-5;
  const double rho = (std::fabs(f - f_new) < 1e-15 || std::fabs(pred) < 1e-15) ? 0.5 : (f - f_new) / pred;
  const bool search_each = mode == GPSLAM_DOGLEG_SEARCH_EACH_ITERATION, one_step = mode == GPSLAM_DOGLEG_ONE_STEP_PER_ITERATION;
  const bool fin = std::isfinite(rho);       // (an infinite rho of either sign is a trial that went nowhere: the last branch)
  if (fin && rho >= 0.75) {
    const double nd = std::fmax(*delta, 3.0 * norm);
    *keep = 1;
    if (!search_each || std::fabs(nd - *delta) < 1e-15 || *last_action == 2) *stay = 0;
    else { *stay = 1; *last_action = 1; }
    *delta = nd;
  } else if (fin && rho >= 0.25) {
    *keep = 1; *stay = 0;
  } else if (fin && rho >= 0.0) {
    const bool floor_hit = !(*delta > kFloor);
    *keep = 1;
    if (one_step || *last_action == 1 || floor_hit) *stay = 0;
    else { *stay = 1; *last_action = 2; }
    if (!floor_hit) *delta *= 0.5;
  } else {                                      // the cost went up, or rho is not a number
    *keep = 0;
    if (*delta > kFloor) { *delta *= 0.5; *stay = 1; *last_action = 2; }
    else *stay = 0;
  }
  return 0;
}

int gpslam_hip_iterate_dogleg(gpslam_hip_handle *h, double *delta, int32_t mode, gpslam_hip_stats *st) {
  if (!h || !delta || !(*delta > 0.0) || !std::isfinite(*delta) || !dl_mode_ok(mode)) return GPSLAM_E_INVALID;
  int rc = dl_guard(h, "iterate_dogleg");
  if (rc) return rc;
  h->mg.invalidate();
  return dl_iterate(h, delta, mode, st);
}

int gpslam_hip_optimize_dogleg(gpslam_hip_handle *h, const gpslam_hip_params *p, double delta_initial, int32_t mode, gpslam_hip_stats *st) {
  if (!h || !p || !(delta_initial > 0.0) || !std::isfinite(delta_initial) || !dl_mode_ok(mode)) return GPSLAM_E_INVALID;
  int rc = dl_guard(h, "optimize_dogleg");
  if (rc) return rc;
  h->mg.invalidate();
  // NonlinearOptimizer::defaultOptimize: do { cur = error(); iterate(); } while (!converged)
  double err0;
  if ((rc = impl64::gpslam_hip_error(h, &err0))) return rc;
  gpslam_hip_stats it;
  std::memset(&it, 0, sizeof(it));
  double new_err = err0, dinf = 0.0, delta = delta_initial;
  int iters = 0;
  if (!(err0 <= p->error_tol)) {
    for (;;) {
      const double cur = new_err;
      if ((rc = dl_iterate(h, &delta, mode, &it))) break;
      iters++;
      new_err = it.error_after;
      dinf = it.delta_inf_norm;
      if (iters >= p->max_iterations) break;
      if (new_err <= p->error_tol) break;
      const double abs_dec = cur - new_err, rel_dec = abs_dec / cur;
      if (rel_dec <= p->relative_error_tol || abs_dec <= p->absolute_error_tol) break;
      if (p->delta_tol > 0.0 && dinf < p->delta_tol) break;
    }
  }
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->error_before = err0; st->error_after = new_err; st->delta_inf_norm = dinf;
    st->iterations = iters; st->status = rc; st->lambda = delta;
    // of the last iteration that ran (zero when none did, or when it failed)
    st->accepted = (iters > 0 && !rc) ? it.accepted : 0;
    st->trials = it.trials; st->last_trial_error = iters > 0 ? it.last_trial_error : err0;
  }
  return rc;
}

int gpslam_hip_dogleg_last(gpslam_hip_handle *h, double *out8) {
  if (!h || !out8) return GPSLAM_E_INVALID;
  for (int i = 0; i < 8; i++) out8[i] = h->dl.last[i];
  return 0;
}

}  // extern "C"
