// qc_learn.hip -- learning Qc from data (include/gpslam_hip_qc.h): the statistic
//   A = sum_i sum_{k = 1, 2} ( e~_k e~_k^T + J~_k Sigma_J J~_k^T ),    n_f = the number of GP priors summed,
// over the GP priors that carry the handle's shared Qc, from what gpslam_hip_marginals left on the device (Sigma_{i,i} in mg.S,
// Sigma_{i,i+1} in mg.Sn), and the host arithmetic on it: G = n_f Qc - A / 2 (the derivative of the log-evidence in W = Qc^-1 at fixed
// states), the EM update Qc+ = A / (2 n_f), the stationary scale theta+ = tr(Qc0^-1 A) / (2 n_f d).
//   (a) k_qc_stat<MF, VW>: one wave per workgroup, a contiguous run of priors each.  A stage of 64 priors is evaluated one prior per
//       lane with the device functions of gp_block (GpPrior::eval; SE(3): the form of gp_pose3_rows with U = I, which never holds the
//       12 x 24 Jacobian) and waits in the lanes' registers; in rounds of 16 the lanes deposit the time-whitened J~ (2d x 4d) and e~ (2d)
//       of their prior in LDS (64 slots of SE(3) would be 154 KB).  Then, prior by prior of the round,
//       the wave reads S_i, Sn_i, S_{i+1} as three whole coalesced blocks (the next prior's are asked for before this one's products),
//       lays Sigma_J out in LDS, forms P = J~ Sigma_J with the lanes over P's entries, and the d x d contribution
//       sum_k (e~_k e~_k^T + P_k J~_k^T) with the lanes over its entries -- each lane keeps ONE running entry of A in a register.  No
//       thread ever holds Sigma_J (576 doubles at b = 12).  The products are plain fp64 FMAs (VALU): the MFMA form was not built, see
//       DESIGN 4k.  It writes nothing but its partial: the solver's buffers and the marginals stay as they are;
//   (b) k_qc_reduce: one workgroup adds the partials in a tree of fixed shape (as k_ev_reduce) and writes 1/2 (A + A^T).
// fp64 only; no atomics, every sum in a fixed order, the grid a function of the prior count alone: two calls give the same bits.
#include "api_common.hpp"
#include "../../include/gpslam_hip_qc.h"

#include <cmath>

namespace {

// A stage: 64 priors, one per lane, evaluated into registers.  A round: the 16 of them whose J~ and e~ the LDS holds at a time.  The
// stride of one prior's slot: 2d x 4d + 2d doubles, made odd so that the lanes' slots start in different banks
constexpr int kQcStage = 64, kQcRound = 16;
constexpr int qc_js(int d) { return (2 * d * 4 * d + 2 * d) | 1; }
constexpr int kQcMaxWorkgroups = 2048;    // beyond that many stages a workgroup takes several, one after the other
constexpr int kQcReduceThreads = 256;

struct QcStat {
  const double *pose, *vel;     // SoA
  int stride;
  const int *left;              // device order (compile() sorts by Qc: the shared-Qc priors lead)
  const double *dt;
  int count;                    // the shared-Qc priors: device positions 0 .. count - 1
  const double *S, *Sn;         // mg.S, mg.Sn: N x b x b
  int per_wg;                   // priors per workgroup, a multiple of the stage
  double *part;                 // gridDim.x x d x d
};

// One prior's linearisation, held in the registers of the lane that evaluated it until its turn to deposit J~ (rows k d + r, k = 0, 1;
// 4d columns) and e~ (behind it) in an LDS slot.  The generic form: the d <= 3 manifolds hold Jt, Jb (2 x d x 4d <= 72 doubles)
template <int MF> struct QcLin {
  static constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, W = 4 * d;
  double e[2 * d], Jt[d * W], Jb[d * W], sa, sb, sc;
  __device__ __forceinline__ void compute(const QcStat &a, int f) {
    const int i = a.left[f];
    const double dt = a.dt[f];
    double p1[pd], p2[pd], v1[d], v2[d];
#pragma unroll
    for (int k = 0; k < pd; k++) { p1[k] = a.pose[(size_t)k * a.stride + i]; p2[k] = a.pose[(size_t)k * a.stride + i + 1]; }
#pragma unroll
    for (int k = 0; k < d; k++) { v1[k] = a.vel[(size_t)k * a.stride + i]; v2[k] = a.vel[(size_t)k * a.stride + i + 1]; }
    GpPrior<double, MF, true>::eval(p1, v1, p2, v2, dt, e, Jt, Jb);
    const double sq = sqrt(dt);
    sa = 3.4641016151377545870548926830117 / (dt * sq);   // sqrt(12 / dt^3): gp_block's scalars
    sb = -1.7320508075688772935274463415059 / sq;
    sc = 1.0 / sq;
  }
  __device__ __forceinline__ void deposit(const QcStat &, int, double *out) const {
#pragma unroll
    for (int r = 0; r < d; r++) {
#pragma unroll
      for (int c = 0; c < W; c++) {
        out[r * W + c] = sa * Jt[r * W + c] + sb * Jb[r * W + c];
        out[(d + r) * W + c] = sc * Jb[r * W + c];
      }
      out[2 * d * W + r] = sa * e[r] + sb * e[d + r];
      out[2 * d * W + d + r] = sc * e[d + r];
    }
  }
};

// SE(3): gp_pose3_rows without the Qc half of the whitening (U = I).  What waits in registers is what the 12 x 24 Jacobian is a
// function of -- Jinv = Jr^-1(r), FD = d(Jinv v2)/dr, J = -Jinv Ad(h^-1), three block lower-triangular 6 x 6 (81 doubles) -- and the
// rows are formed as they are deposited: [H3 H4] = [[Jinv, 0], [FD Jinv, Jinv]], [H1 H2] = [[J, -dt I], [FD J, -I]]
template <bool VW> struct QcLinPose3 {
  static constexpr int W = 24;
  BL6<double> Jinv, FD, J;
  double et[12], sa, sb, sc, dt;
  __device__ __forceinline__ void compute(const QcStat &a, int f) {
    const int i = a.left[f];
    dt = a.dt[f];
    double q1[12], q2[12], w1[6], w2[6];
#pragma unroll
    for (int k = 0; k < 12; k++) { q1[k] = a.pose[(size_t)k * a.stride + i]; q2[k] = a.pose[(size_t)k * a.stride + i + 1]; }
#pragma unroll
    for (int k = 0; k < 6; k++) { w1[k] = a.vel[(size_t)k * a.stride + i]; w2[k] = a.vel[(size_t)k * a.stride + i + 1]; }
    if constexpr (VW) {   // GaussianProcessPriorPose3VW.h:87-88: body velocities of the world-frame (v, w)
      double b1[6], b2[6];
      vw_to_vb(q1, w1, b1);
      vw_to_vb(q2, w2, b2);
#pragma unroll
      for (int k = 0; k < 6; k++) { w1[k] = b1[k]; w2[k] = b2[k]; }
    }
    const SE3<double> h = se3_between(as_se3(q1), as_se3(q2));
    const V6<double> r = se3_log(h);
    const JrK<double> k0 = jr_coefs(r.w);
    Jinv = se3_jrinv_k(k0, r);
    const V6<double> u1 = as_v6(w1), u2 = as_v6(w2);
    const double sq = sqrt(dt);
    sa = 3.4641016151377545870548926830117 / (dt * sq);
    sb = -1.7320508075688772935274463415059 / sq;
    sc = 1.0 / sq;
    const V6<double> top = r - dt * u1;
    const V6<double> bot = Jinv * u2 - u1;
    const double e[12] = {top.w.x, top.w.y, top.w.z, top.v.x, top.v.y, top.v.z, bot.w.x, bot.w.y, bot.w.z, bot.v.x, bot.v.y, bot.v.z};
#pragma unroll
    for (int q = 0; q < 6; q++) {
      et[q] = sa * e[q] + sb * e[6 + q];
      et[6 + q] = sc * e[6 + q];
    }
    FD = se3_jrinv_times_x_fd_k(k0, r, u2);
    J = neg(Jinv * se3_adjoint(se3_inverse(h)));
  }
  // rows rho and 6 + rho of one state's 12 columns: the right state [sa X + sb Y | sb X], [sc Y | sc X]; the left one
  // [sa X + sb Y | kt I], [sc Y | kb I]
  template <bool RIGHT>
  __device__ __forceinline__ void half(const BL6<double> &X, const BL6<double> &Y, double kt, double kb, double *out) const {
#pragma unroll
    for (int rho = 0; rho < 6; rho++) {
      double s1[12], s2[12];
#pragma unroll
      for (int c = 0; c < 6; c++) {
        const double x = bl6_at(X, rho, c), y = bl6_at(Y, rho, c);
        s1[c] = sa * x + sb * y;
        s2[c] = sc * y;
        if (RIGHT) { s1[6 + c] = sb * x; s2[6 + c] = sc * x; }
        else { s1[6 + c] = c == rho ? kt : 0.0; s2[6 + c] = c == rho ? kb : 0.0; }
      }
#pragma unroll
      for (int c = 0; c < 12; c++) { out[rho * W + (RIGHT ? 12 : 0) + c] = s1[c]; out[(6 + rho) * W + (RIGHT ? 12 : 0) + c] = s2[c]; }
    }
  }
  __device__ __forceinline__ void deposit(const QcStat &a, int f, double *out) const {
#pragma unroll
    for (int q = 0; q < 12; q++) out[12 * W + q] = et[q];
    half<true>(Jinv, FD * Jinv, 0.0, 0.0, out);
    half<false>(J, FD * J, -(sa * dt + sb), -sc, out);
    if constexpr (VW) {
      // the rows above are those of the body-velocity factor; each state's 12 columns of every row go through vw_row_transform
      // in place, row by row (the rotations and the body velocities are read again here, not kept next to the three blocks)
      const int i = a.left[f];
#pragma unroll 1
      for (int s = 0; s < 2; s++) {
        double p[9], w[6], v[6];
#pragma unroll
        for (int k = 0; k < 9; k++) p[k] = a.pose[(size_t)k * a.stride + i + s];
#pragma unroll
        for (int k = 0; k < 6; k++) w[k] = a.vel[(size_t)k * a.stride + i + s];
        vw_to_vb(p, w, v);
#pragma unroll 1
        for (int row = 0; row < 12; row++) {
          double seg[12];
#pragma unroll
          for (int c = 0; c < 12; c++) seg[c] = out[row * W + 12 * s + c];
          vw_row_transform(p, v, seg);
#pragma unroll
          for (int c = 0; c < 12; c++) out[row * W + 12 * s + c] = seg[c];
        }
      }
    }
  }
};

template <int MF, bool VW> __global__ void __launch_bounds__(64) k_qc_stat(QcStat a) {
  constexpr int d = MTraits<MF>::d, b = 2 * d, W = 4 * d, DD = d * d, BB = b * b;
  constexpr int NPW = kQcRound, JS = qc_js(d);
  constexpr int NS = (3 * BB + 63) / 64, NPE = (2 * d * W + 63) / 64;
  using Lin = typename std::conditional<MF == POSE3, QcLinPose3<VW>, QcLin<MF == POSE3 ? LINEAR3 : MF>>::type;
  __shared__ double Jl[NPW * JS], Sig[W * W], P[2 * d * W];
  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * a.per_wg, g1 = min(g0 + a.per_wg, a.count);
  double pre[NS];
  auto fetch = [&](int f) {       // S_i, Sn_i, S_{i+1}: three whole blocks, consecutive lanes on consecutive doubles
    const size_t i = (size_t)a.left[f];
#pragma unroll
    for (int t = 0; t < NS; t++) {
      const int idx = lane + 64 * t;
      pre[t] = 0.0;
      if (idx < 3 * BB) {
        const int blk = idx / BB, e = idx - blk * BB;
        const double *src = blk == 1 ? a.Sn + i * BB : a.S + (i + (blk >> 1)) * BB;
        pre[t] = src[e];
      }
    }
  };
  double acc = 0.0;               // lane r d + s < d d: entry (r, s) of this workgroup's partial
  for (int s0 = g0; s0 < g1; s0 += kQcStage) {
    const int ns = min(kQcStage, g1 - s0);
    Lin lin;
    const int mine = min(s0 + lane, g1 - 1);    // (a lane past the end repeats the last prior: in bounds, never deposited)
    lin.compute(a, mine);
#pragma unroll 1
    for (int q0 = 0; q0 < ns; q0 += NPW) {
      const int np = min(NPW, ns - q0);
      __syncthreads();            // (the last round's J~ has been read)
      if (lane >= q0 && lane < q0 + np) lin.deposit(a, mine, Jl + (lane - q0) * JS);
      fetch(s0 + q0);
      for (int p = 0; p < np; p++) {
        const double *Jp = Jl + p * JS;
#pragma unroll
        for (int t = 0; t < NS; t++) {          // Sigma_J = [[S_i, Sn_i], [Sn_i^T, S_{i+1}]]
          const int idx = lane + 64 * t;
          if (idx < 3 * BB) {
            const int blk = idx / BB, e = idx - blk * BB, r = e / b, c = e - r * b;
            if (blk == 0) Sig[r * W + c] = pre[t];
            else if (blk == 2) Sig[(b + r) * W + b + c] = pre[t];
            else { Sig[r * W + b + c] = pre[t]; Sig[(b + c) * W + r] = pre[t]; }
          }
        }
        __syncthreads();
        if (p + 1 < np) fetch(s0 + q0 + p + 1);
        double v[NPE];
#pragma unroll
        for (int t = 0; t < NPE; t++) {         // P = J~ Sigma_J
          const int o = lane + 64 * t;
          v[t] = 0.0;
          if (o < 2 * d * W) {
            const int r = o / W, c = o - r * W;
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < W; q++) s += Jp[r * W + q] * Sig[q * W + c];
            v[t] = s;
          }
        }
#pragma unroll
        for (int t = 0; t < NPE; t++) {         // (P was last read before the barrier above)
          const int o = lane + 64 * t;
          if (o < 2 * d * W) P[o] = v[t];
        }
        __syncthreads();
        if (lane < DD) {
          const int r = lane / d, s = lane - r * d;
#pragma unroll
          for (int k = 0; k < 2; k++) {
            double t = Jp[2 * d * W + k * d + r] * Jp[2 * d * W + k * d + s];
#pragma unroll
            for (int c = 0; c < W; c++) t += P[(k * d + r) * W + c] * Jp[(k * d + s) * W + c];
            acc += t;
          }
        }
      }
    }
  }
  if (lane < DD) a.part[(size_t)blockIdx.x * DD + lane] = acc;
}

// A = 1/2 (T + T^T), T the sum of the np partials in a tree of fixed shape: entry e of run t (a contiguous run of partials, in
// order) in thread t d d + e, the runs in order in thread e
__global__ void __launch_bounds__(kQcReduceThreads) k_qc_reduce(const double *part, int np, int d, double *A) {
  __shared__ double red[kQcReduceThreads], tot[36];
  const int tid = threadIdx.x, DD = d * d, runs = kQcReduceThreads / DD;
  const int run = tid / DD, e = tid - run * DD;
  if (run < runs) {
    const int per = (np + runs - 1) / runs, i0 = min(run * per, np), i1 = min(i0 + per, np);
    double acc = 0.0;
    for (int i = i0; i < i1; i++) acc += part[(size_t)i * DD + e];
    red[tid] = acc;
  }
  __syncthreads();
  if (tid < DD) {
    double t = 0.0;
    for (int q = 0; q < runs; q++) t += red[q * DD + tid];
    tot[tid] = t;
  }
  __syncthreads();
  if (tid < DD) {
    const int r = tid / d, c = tid - r * d;
    A[tid] = 0.5 * (tot[r * d + c] + tot[c * d + r]);
  }
}

int qc_refuse(gpslam_hip_handle *h) {
  const char *why = nullptr;
  if (h->cfg.precision == GPSLAM_FP32) why = "fp32 handles are not supported (fp64 only)";
  else if (sharded(h)) why = "sharded handles are not supported";
  else if (h->fs.active && h->fs.split) why = "split pieces are not supported";
  else if (h->mf == ROT3_BIAS) why = "GPSLAM_ROT3_BIAS is not supported (the pad coordinates of its velocity slot carry no Qc)";
  if (why) return fail(h, GPSLAM_E_UNSUPPORTED, (std::string("qc_statistic: ") + why).c_str());
  return 0;
}

template <int MF> void qc_launch(gpslam_hip_handle *h, const QcStat &a, int nwg) {
  if constexpr (MF == POSE3) {
    if (h->vw) { k_qc_stat<MF, true><<<dim3(nwg), dim3(64), 0, h->stream>>>(a); return; }
  }
  k_qc_stat<MF, false><<<dim3(nwg), dim3(64), 0, h->stream>>>(a);
}

bool qc_sym_spd(int d, const double *M) {
  double C[36];
  for (int i = 0; i < d * d; i++) {
    if (!std::isfinite(M[i])) return false;
    C[i] = M[i];
  }
  return spd_chol_upper(d, C);
}

}  // namespace

extern "C" {

int gpslam_hip_qc_statistic(gpslam_hip_handle *h, double *A, int64_t *n_f) {
  if (!h || !A) return GPSLAM_E_INVALID;
  int rc;
  if ((rc = qc_refuse(h)) || (rc = marginals_getter_check(h))) return rc;
  const int d = h->d, DD = d * d;
  // compile() orders the device-side arrays by Qc with a stable sort: the priors of the shared Qc (gp_q == 0) lead
  int count = 0;
  for (size_t f = 0; f < h->gp_left.size(); f++) count += (f >= h->gp_q.size() || h->gp_q[f] == 0) ? 1 : 0;
  if (n_f) *n_f = count;
  for (int i = 0; i < DD; i++) A[i] = 0.0;
  if (count == 0) return 0;
  (void)hipSetDevice(h->cfg.device);
  const int npw = kQcStage, stages = nblocks(count, npw), spw = nblocks(stages, kQcMaxWorkgroups), nwg = nblocks(stages, spw);
  h->qcl.fit(h->N);
  HIPCHK(h->qcl.part.reserve(((size_t)nwg + 1) * DD * sizeof(double)));     // (the result behind the partials)
  QcStat a;
  a.pose = h->pose.as<double>(); a.vel = h->vel.as<double>(); a.stride = h->stride;
  a.left = h->d_gp_left.as<int>(); a.dt = h->d_gp_dt.as<double>(); a.count = count;
  a.S = h->mg.S.as<double>(); a.Sn = h->mg.Sn.as<double>();
  a.per_wg = spw * npw; a.part = h->qcl.part.as<double>();
  switch (h->mf) {
    case LINEAR2: qc_launch<LINEAR2>(h, a, nwg); break;
    case LINEAR3: qc_launch<LINEAR3>(h, a, nwg); break;
    case POSE2: qc_launch<POSE2>(h, a, nwg); break;
    case POSE3: qc_launch<POSE3>(h, a, nwg); break;
    case ROT3: qc_launch<ROT3>(h, a, nwg); break;
  }
  double *res = a.part + (size_t)nwg * DD;
  k_qc_reduce<<<dim3(1), dim3(kQcReduceThreads), 0, h->stream>>>(a.part, nwg, d, res);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(A, res, DD * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int gpslam_hip_qc_gradient(int32_t d, const double *Qc, const double *A, int64_t n_f, double *G) {
  if (d < 1 || d > 6 || !Qc || !A || !G || n_f <= 0 || !qc_sym_spd(d, Qc)) return GPSLAM_E_INVALID;
  for (int i = 0; i < d * d; i++)
    if (!std::isfinite(A[i])) return GPSLAM_E_INVALID;
  for (int i = 0; i < d * d; i++) G[i] = (double)n_f * Qc[i] - 0.5 * A[i];
  return 0;
}

int gpslam_hip_qc_em_update(int32_t d, const double *A, int64_t n_f, double *Qc_next) {
  if (d < 1 || d > 6 || !A || !Qc_next || n_f <= 0 || !qc_sym_spd(d, A)) return GPSLAM_E_INVALID;
  const double s = 1.0 / (2.0 * (double)n_f);
  for (int r = 0; r < d; r++)
    for (int c = 0; c < d; c++) Qc_next[r * d + c] = 0.5 * (A[r * d + c] + A[c * d + r]) * s;
  return 0;
}

int gpslam_hip_qc_em_scale(int32_t d, const double *Qc0, const double *A, int64_t n_f, double *theta) {
  if (d < 1 || d > 6 || !Qc0 || !A || !theta || n_f <= 0 || !qc_sym_spd(d, A)) return GPSLAM_E_INVALID;
  double C[36];
  for (int i = 0; i < d * d; i++) {
    if (!std::isfinite(Qc0[i])) return GPSLAM_E_INVALID;
    C[i] = Qc0[i];
  }
  if (!spd_chol_upper(d, C)) return GPSLAM_E_INVALID;       // Qc0 = C^T C
  // tr(Qc0^-1 A): column j of Qc0^-1 A by two triangular solves, its entry j added
  double tr = 0.0;
  for (int j = 0; j < d; j++) {
    double y[6], z[6];
    for (int i = 0; i < d; i++) {   // C^T y = A[:, j] (forward)
      double s = 0.5 * (A[i * d + j] + A[j * d + i]);
      for (int k = 0; k < i; k++) s -= C[k * d + i] * y[k];
      y[i] = s / C[i * d + i];
    }
    for (int i = d - 1; i >= 0; i--) {   // C z = y (backward): z = Qc0^-1 A[:, j]
      double s = y[i];
      for (int k = i + 1; k < d; k++) s -= C[i * d + k] * z[k];
      z[i] = s / C[i * d + i];
    }
    tr += z[j];
  }
  *theta = tr / (2.0 * (double)n_f * (double)d);
  return 0;
}

}  // extern "C"
