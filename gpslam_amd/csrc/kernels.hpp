// kernels.hpp -- HIP kernels of the GP-SLAM Gauss-Newton iteration (gfx950, wave64).
//
// HBM data layout (DESIGN.md has the full picture):
//   states      SoA   pose[k * stride + i], vel[k * stride + i]      (coalesced across factors)
//   row table   AoS   one record per whitened Jacobian row: rowLR[rho][2b] = [dL | dR], rowE[rho]
//                     rows are grouped by the LEFT state of their factor; rowptr[s] .. rowptr[s+1]
//   blocks      AoS   per state one record [D (b x b) | O (b x b) | G (R cols of b)], O_s = H[s+1, s]
//                     (k_fused_level0 never writes them: it forms them in LDS)
//   solver      the same records, overwritten in place by the elimination with [V | U | Y]
//
// Kernels:
//   k_gp          batched GaussianProcessPrior*::evaluateError + H1..H4 (+ whitening)     [K1]
//   k_simple      PriorFactor / BetweenFactor rows;  k_meas  measurement factors           [K2]
//   k_assemble_ghost   J^T J / J^T e per state from the row table (no atomics, fixed order) [K3]
//   k_lm_*        landmark border: Schur complement on the chain solution                 [K5]
//   k_interp_query     batched interpolatePose of the current estimate
//   k_chunk_forward / k_chunk_backward   partitioned block Gauss-Jordan, one wave per chunk,
//                 one panel column per lane, pivot broadcast through v_readlane            [K4]
//   k_chunk_forward_rows   level 0 for block size 12: four chunks per wave on 16-lane DPP rows, panel ROWS in lanes,
//                 pivot rows by v_mov_b64_dpp row_newbcast                                  [K4]
//   k_fused_level0     K3 inside K4 level 0: two-wave workgroups, one wave assembles the block records of four
//                 chunks from the row tables, the other eliminates them (LDS hand-over)      [K3 + K4]
//   k_retract     x <- x (+) delta, |delta|_inf                                            [K6]
// k_chunk_forward_rows, k_fused_level0 and k_chunk_backward_rows are level0.hpp's, compiled by level0.hip alone; their argument
// structs and the declarations of their launchers are here, so every unit that includes this file can fill and call without
// compiling a form of them.
#pragma once

#include <hip/hip_runtime.h>

#include "factors.hpp"
#include "dpp.hpp"
#include "cr_step.hpp"
#include "cr_quad.hpp"
#include "robust.hpp"
#include <type_traits>

namespace gps {

constexpr int kMaxRhs = 28;  // 3B + R <= 64 for B = 12

template <typename T> struct UMat { T u[36]; };  // chol_upper(Qc^-1), d x d row-major

// ------------------------------------------------------------------ reductions

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
// |v| for a maximum that must not lose NaNs (fmax drops them): a NaN update reads as +inf
template <typename T> __device__ __forceinline__ T abs_or_inf(T v) { return (v == v) ? fabs(v) : T(INFINITY); }
template <typename T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  return v;
}
// block-wide sum (blockDim.x multiple of 64, <= 256); result valid in thread 0
template <typename T> __device__ __forceinline__ T block_sum(T v) {
  __shared__ T red[4];
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  T r = T(0);
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)((blockDim.x + 63) >> 6); i++) r += red[i];
  return r;
}
template <typename T> __device__ __forceinline__ T block_max(T v) {
  __shared__ T redm[4];
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) redm[w] = v;
  __syncthreads();
  T r = T(0);
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)((blockDim.x + 63) >> 6); i++) r = fmax(r, redm[i]);
  return r;
}

// out[slot] = sum (mode 0) or max (mode 1) of in[0..n), single block, fixed order -> deterministic
// (round 6: a thread's operands are requested sixteen at a time and then added in the order they always were -- the error partials of
//  a 1e6-state graph with measurement factors are 47 000 numbers, 183 dependent load round trips per thread: 40-70 us of config 5's
//  SE(3) iteration, 2.5 x 20 us of config 4's)
template <typename T, int NT = 256> __device__ __forceinline__ T strided_fold(const T *in, int n, int mode) {
  T acc = T(0);
  int i = threadIdx.x;
  for (; i + 15 * NT < n; i += 16 * NT) {
    T v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = in[i + u * NT];
#pragma unroll
    for (int u = 0; u < 16; u++) acc = mode ? fmax(acc, v[u]) : acc + v[u];
  }
  for (; i < n; i += NT) acc = mode ? fmax(acc, in[i]) : acc + in[i];
  return acc;
}
template <typename T> __global__ void __launch_bounds__(256) k_final_reduce(const T *in, int n, double *out, int mode) {
  const T acc = strided_fold(in, n, mode);
  const T r = mode ? block_max(acc) : block_sum(acc);
  if (threadIdx.x == 0) *out = (double)r;
}


// ------------------------------------------------------------------ K1: GP prior rows

// fp32 arithmetic only: every factor here is invariant under a common translation of the variables it touches, and the
// states sit in HBM as fp64.  Before the arithmetic drops to float the translations are re-centred on the factor's
// first pose IN FP64, so that a Jacobian computed 1e5 m from the origin is as accurate as one computed at the origin
// (a float holds 1e5 m to 8 mm: the 0.1 m step between consecutive states would carry 4 digits).  The fp64
// instantiations do not re-centre: their results stay bit-identical to what the oracle parity tests pinned.
// (LINEAR3 is (x, y, theta) for OdometryFactor2DLinear / RangeBearingFactor2DLinear, whose Jacobians are evaluated AT theta:
//  only x and y are re-centred -- ADVICE r2; a plain GaussianProcessPriorLinear<3> chain loses nothing by that, its Jacobians
//  are constants.)
template <int MF> struct TransPart {
  static constexpr int n = (MF == POSE3) ? 3 : ((MF == POSE2 || MF == LINEAR3) ? 2 : ((MF == ROT3 || MF == ROT3_BIAS) ? 0 : MTraits<MF>::pd));
  static constexpr int off = (MF == POSE3) ? 9 : 0;
};
template <typename T> struct IsF64 { static constexpr bool v = false; };
template <> struct IsF64<double> { static constexpr bool v = true; };

// Inputs (states, landmarks, factor parameters) are ALWAYS fp64 in HBM; T is the arithmetic / row-table type.  In the
// fp32 mode (GPSLAM_FP32) the Jacobian rows are computed and stored with T = float; the normal equations and the solver stay
// double (api_impl.inc: Real), and the residual is evaluated by the T = double error pass of the same kernels, which then also
// deposits its whitened error, rounded once, as the row tables' right-hand side (rowE32): fp32 Jacobians + fp64 residual =
// iterative refinement through the Gauss-Newton loop.
// Pending update (round 5).  Inside a fixed-count Gauss-Newton run the retraction of iteration k is folded into the linearisation
// of iteration k + 1: K1 reads a state, applies the update the previous solve left in the level-0 solution array, linearises at the
// updated values, and the thread that OWNS the state (the GP prior whose left state it is; the last state rides with the last
// factor) writes it into the OTHER state buffer -- the host swaps the two buffers behind the launch.  One launch (k_retract) and one
// read + write of every state less per iteration; Values::retract and NonlinearFactorGraph::linearize of GaussNewtonOptimizer::iterate
//  in one pass over the states.  The same arithmetic in the same order as k_retract: bit-identical states.
struct PendUpd {
  const double *dx = nullptr;   // N x b updates (level-0 solutions, R = 1), or null: nothing pending
  double *pose_w = nullptr, *vel_w = nullptr;   // the other state buffer (same SoA stride)
  const int *flag = nullptr;    // non-SPD flag of the solve that produced dx: set -> the states stay as they are
  int chart = 0, last = 0;      // retract chart; index of the chain's last state
};
// state i as K1 sees it: the stored value, or -- with an update pending -- its retraction; `own`: this thread writes it back
template <int MF> __device__ __forceinline__ void load_state_upd(const double *pose, const double *vel, int stride, int i, const PendUpd &u,
                                                                  bool own, double *p, double *v) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, b = 2 * d;
#pragma unroll
  for (int k = 0; k < pd; k++) p[k] = pose[(size_t)k * stride + i];
#pragma unroll
  for (int k = 0; k < d; k++) v[k] = vel[(size_t)k * stride + i];
  if (u.dx != nullptr) {
    if (!*u.flag) {
      double dl[b], q[pd];
#pragma unroll
      for (int k = 0; k < b; k++) dl[k] = u.dx[(size_t)i * b + k];
      PoseFactors<double, MF, false>::retract(p, dl, u.chart, q);
#pragma unroll
      for (int k = 0; k < pd; k++) p[k] = q[k];
#pragma unroll
      for (int k = 0; k < d; k++) v[k] += dl[d + k];
    }
    if (own) {
#pragma unroll
      for (int k = 0; k < pd; k++) u.pose_w[(size_t)k * stride + i] = p[k];
#pragma unroll
      for (int k = 0; k < d; k++) u.vel_w[(size_t)k * stride + i] = v[k];
    }
  }
}
// states i and i + 1 of a two-state factor the same way, every request in flight before the first one is waited for (round 6): the
// single-state form behind a branch on the solve's flag put four dependent memory round trips in front of K1's arithmetic -- state,
// flag, update, and the same again for the right state -- 11 of a K1 wave's 33 us (scripts/trace_klin.py)
template <int MF> __device__ __forceinline__ void load_two_states_upd(const double *pose, const double *vel, int stride, int i, const PendUpd &u,
                                                                      bool own1, bool own2, double *p1, double *v1, double *p2, double *v2) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, b = 2 * d;
#pragma unroll
  for (int k = 0; k < pd; k++) { p1[k] = pose[(size_t)k * stride + i]; p2[k] = pose[(size_t)k * stride + i + 1]; }
#pragma unroll
  for (int k = 0; k < d; k++) { v1[k] = vel[(size_t)k * stride + i]; v2[k] = vel[(size_t)k * stride + i + 1]; }
  if (u.dx != nullptr) {
    const int bad = *u.flag;
    double dl1[b], dl2[b];
#pragma unroll
    for (int k = 0; k < b; k++) { dl1[k] = u.dx[(size_t)i * b + k]; dl2[k] = u.dx[(size_t)(i + 1) * b + k]; }
    if (!bad) {
      double q[pd];
      PoseFactors<double, MF, false>::retract(p1, dl1, u.chart, q);
#pragma unroll
      for (int k = 0; k < pd; k++) p1[k] = q[k];
#pragma unroll
      for (int k = 0; k < d; k++) v1[k] += dl1[d + k];
      PoseFactors<double, MF, false>::retract(p2, dl2, u.chart, q);
#pragma unroll
      for (int k = 0; k < pd; k++) p2[k] = q[k];
#pragma unroll
      for (int k = 0; k < d; k++) v2[k] += dl2[d + k];
    }
    if (own1) {
#pragma unroll
      for (int k = 0; k < pd; k++) u.pose_w[(size_t)k * stride + i] = p1[k];
#pragma unroll
      for (int k = 0; k < d; k++) u.vel_w[(size_t)k * stride + i] = v1[k];
    }
    if (own2) {
#pragma unroll
      for (int k = 0; k < pd; k++) u.pose_w[(size_t)k * stride + i + 1] = p2[k];
#pragma unroll
      for (int k = 0; k < d; k++) u.vel_w[(size_t)k * stride + i + 1] = v2[k];
    }
  }
}

template <typename T> struct GpArgs {
  PendUpd pend;                // fp64 SE(3) record launches inside run_gn: the previous iteration's update, applied here
  const double *pose, *vel;    // SoA
  int stride;             // SoA stride (>= N + 1)
  int count;
  const int *left;        // left state of factor f
  const double *dt;
  const int *row0;        // first row of factor f in the row table
  float *rowE32;          // MODE 1 (error only, T = double): also store the whitened error here, or null
  T *rowLR, *rowE;        // MODE 0
  T *partial;             // per-block error partial sums
  T *out_e, *out_H;       // MODE 2: API layout
  UMat<T> U;
  int vw;                 // Pose3 only: velocities are world-frame [v; w] (the *Pose3VW factors)
  T *gps;                 // Pose3, MODE 0: structured records (kGps* below) instead of rows in rowLR / rowE, or null
};

// Structured record of one GaussianProcessPriorPose3 (what k_fused_level0's assembly wave reads when K1 feeds it directly).
// Round 4: the record holds what the whitened 12 x 24 Jacobian [L | R] is a FUNCTION of, not its columns.  With
//   X = Jinv = Jr^-1(r) = [[XA, 0], [XC, XA]]                      (GaussianProcessPriorPose3.h:76; 18 distinct entries)
//   J = Hlog Hcomp1 Hinv = -Jinv Ad(h^-1) = [[JA, 0], [JC, JA]]   (:79-84; the product of two such matrices is one again)
//   F = FD = d(Jinv v2)/dr by central differences = [[FA, 0], [FC, FD]]     (:81, :90; Pose3utils.cpp:167-179; 27 entries)
// the Jacobian is H1 = [J; F J], H2 = [-dt I; -I], H3 = [X; F X], H4 = [0; X] (:79-95), whitened by
// R_w = [[sa U, sb U], [0, sc U]], U = chol_upper(Qc^-1) the same for every factor.  Column c of the whitened halves is
//   L[:, c] = [U (sa J_c + sb F J_c); sc U F J_c]        c < 6 (pose)         [k2 U_c'; -sc U_c']           velocity column c'
//   R[:, c] = [U (sa X_c + sb F X_c); sc U F X_c]                              [sb U X_c'; sc U X_c']
// which the assembly wave forms lane by lane (lane c of a chunk's 16-lane DPP row holds column c): two 6 x 6 matrix-vector
// products with F and four with U per lane and state, all as v_fmac_f64_dpp blocks.  80 doubles = five 128-byte lines per
// factor instead of the 196 doubles of round 2/3's column records (and the 312 of plain rows + errors):
//   [0..8] XA  [9..17] XC  [18..26] JA  [27..35] JC  [36..44] FA  [45..53] FC  [54..62] FD   (3 x 3 blocks, row-major)
//   [63] 0 (the velocity lanes take their zero coefficients from here)
//   [64..75] whitened error,  [76] k2 = -(sa dt + sb), [77] sb, [78] sc, [79] sa
// K1 stages 16 doubles per lane and wave and writes whole 128-byte lines (wave_store_part): the order above is the order in
// which it produces the blocks.  Record F (one past the last factor) is all zeros: states without a GP prior read it.
constexpr int kLinWaves = 2;   // two K1 waves per SIMD (<= 256 VGPRs): linearise phase 87.8 vs 93.3 us with structured records
// The same idea for the d = 3 manifolds (SE(2), SO(3), 3-D linear: block size 6; round 4).  There H1 = [J1; 0], H3 = [J3; 0] and
// H2 = [h2t I; h2b I], H4 = [0; h4b I] with constants (GaussianProcessPriorPose2.h:76-79, GaussianProcessPriorRot3.h:73-76,
// GaussianProcessPriorLinear.h:72-81), so of the whitened 6 x 12 Jacobian only two 3 x 3 blocks are data:
//   [0..8] A1 = U (sa J1)   [9..17] A3 = U (sa J3)   (row-major)        rows 0..2: [A1 | kLt U | A3 | kRt U]
//   [18..23] whitened error   [24] kLt [25] kRt [26] kLb [27] kRb      rows 3..5: [ 0 | kLb U |  0 | kRb U]
//   [28..31] 0                                                           (kLt = sa h2t + sb h2b, kRt = sb h4b, kLb = sc h2b, kRb = sc h4b)
// 32 doubles = two 128-byte lines per factor instead of 6 rows x 13 doubles = 624 bytes written as 96-byte fragments (1.45x write
// amplification measured: profiles/round4_c4_v0).  Consumers: k_assemble_ghost<6> and k_fused_level0<1, double, 6>.
constexpr int kGp3Len = 32, kGp3A1 = 0, kGp3A3 = 9, kGp3E = 18, kGp3S = 24;
// BetweenFactor<Pose3>(x_i, x_i+1) of a chain that runs the structured path (round 4): e = Log(measured^-1 x_i^-1 x_i+1),
// H2 = Jr^-1(e) = [[RA, 0], [RC, RA]], H1 = -Jr^-1(e) Ad((x_i^-1 x_i+1)^-1) = [[LA, 0], [LC, LA]] (GTSAM BetweenFactor.h through
// Pose3::between / Logmap; call site matlab/PlazaPose2.m:125), rows weighted by 1 / sigma:
//   [0..8] RA  [9..17] RC  [18..26] LA  [27..35] LC  (3 x 3, row-major)   [36..41] 1 / sigma   [42..47] whitened error
// 48 doubles = three whole lines instead of six compact rows of 12 + 1 doubles (624 bytes in 96-byte fragments).  The assembly wave
// of k_fused_level0 builds column c of [H1 | H2] in lane c < 6 exactly as it builds the columns of the GP prior's J and X.
constexpr int kBtwLen = 48, kBtwRA = 0, kBtwRC = 9, kBtwLA = 18, kBtwLC = 27, kBtwW = 36, kBtwE = 42;
// Interpolated measurement rows of an SE(3) chain on the structured path (round 5; GPInterpolatedGPSFactorPose3.h:66-95 over
// GaussianProcessInterpolatorPose3.h:82-98).  A whitened row of such a factor is  w Hp [H1 H2 | H3 H4]  with
//   H1 = Ad(Exp(xi)^-1) + He (p11 J + p12 F J),  H2 = l12 He,  H3 = He (p11 X + p12 F X),  H4 = p12 He X
// where X = Jr^-1(r), J = -X Ad(h^-1) and F = d(X v2)/dr are the interval's GP record (kGps*) and l12, p11, p12 the interpolation
// coefficients of tau.  With mu = w Hp He (6) the row is
//   L = [ Lp | l12 mu ],   R = [ mu (p11 X + p12 F X) | p12 mu X ],   Lp = w Hp Ad(Exp(xi)^-1) + mu (p11 J + p12 F J)
// so k_meas writes ONE 128-byte line per row -- [Lp (6) | mu (6) | whitened error, p11, p12, l12] -- instead of 24 + 1 doubles, and
// the assembly wave of k_fused_level0<4> forms R from mu and the X / F X columns it holds for the GP prior anyway: lane c < 16 of
// a chunk's DPP row loads element c of the line (one load per row and lane), mu travels by row_newbcast from lanes 6..11, the four
// scalars from lanes 12..15.
constexpr int kIRowLen = 16, kIRowLp = 0, kIRowMu = 6, kIRowE = 12, kIRowP11 = 13, kIRowP12 = 14, kIRowL12 = 15;
constexpr int kGpsLen = 80, kGpsXA = 0, kGpsXC = 9, kGpsJA = 18, kGpsJC = 27, kGpsFA = 36, kGpsFC = 45, kGpsFD = 54, kGpsZ = 63,
              kGpsE = 64, kGpsS = 76;

// Cooperative row store: every lane of a wave has deposited one row (W doubles, W even) of ITS factor in the wave's
// LDS staging buffer; the wave then writes the 64 rows as 16-byte pieces, consecutive lanes on consecutive pieces of
// the same row, so that each store instruction covers whole 64-byte sectors instead of 64 scattered 16-byte
// fragments (per-lane row stores are store-issue bound and write 2.4x the bytes to HBM: profiles/round1_v2).
// srow[l] = first row of lane l's factor in the row table, or -1.
// wave_store_part: the lanes staged HW (even) doubles each with stride HW + 2; they land at columns
// [coloff, coloff + HW) of row (first row of the lane's factor) + roff of a table with W doubles per row.
template <typename T, int W, int HW, int LS = HW + 2, bool STREAM = false>
__device__ __forceinline__ void wave_store_part(const T *st, const int *srow, int lane, int roff, int coloff, T *table) {
  constexpr int P = HW / 2;
  typedef T V2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int t = 0; t < P; t++) {
    const int q = t * 64 + lane;
    const int fl = q / P, piece = q - fl * P;
    const int r0 = srow[fl];
    if (r0 >= 0) {
      const V2 v = *reinterpret_cast<const V2 *>(st + fl * LS + piece * 2);
      V2 *dst = reinterpret_cast<V2 *>(table + (size_t)(r0 + roff) * W + coloff + piece * 2);
      // STREAM (the structured records: written once in whole 128-byte lines, read once by the next launch): 1e6 Pose3 states
      // K1 0.376 -> 0.337 ms, 1e5: the iteration -5..-12 us.  Not for row tables: their 16-byte fragments of 96-byte half rows
      // had DOUBLED K1 with this hint (round 2); the factor records of k_fused_level0 and the solutions of the
      // back-substitution, which the next launch finds in the caches, lose 3 and 20 us of the iteration with it.
      if constexpr (STREAM) __builtin_nontemporal_store(v, dst);
      else *dst = v;
    }
  }
}
template <typename T, int W>
__device__ __forceinline__ void wave_store_rows(const T *st, const int *srow, int lane, int roff, T *table) {
  wave_store_part<T, W, W>(st, srow, lane, roff, 0, table);
}
// HW consecutive scalars per lane (stride HW + 2) to table[first row + k]: 8-byte pieces (the first row may be odd)
template <typename T, int HW>
__device__ __forceinline__ void wave_store_scalars(const T *st, const int *srow, int lane, T *table) {
  constexpr int LS = HW + 2;
#pragma unroll
  for (int t = 0; t < HW; t++) {
    const int q = t * 64 + lane;
    const int fl = q / HW, k = q - fl * HW;
    const int r0 = srow[fl];
    if (r0 >= 0) table[r0 + k] = st[fl * LS + k];
  }
}

// Row rho of U * M, U upper triangular d x d (row-major, d = 6), M block lower-triangular [[A, 0], [C, D]]:
// only the structurally non-zero products are formed.
template <typename T>
__device__ __forceinline__ void utri_times_bl6_row(const T *U, const BL6<T> &M, int rho, T *out) {
#pragma unroll
  for (int c = 0; c < 6; c++) {
    T acc = T(0);
#pragma unroll
    for (int r = 0; r < 6; r++) {
      if (r < rho) continue;
      if (r < 3 && c >= 3) continue;
      acc += U[rho * 6 + r] * bl6_at(M, r, c);
    }
    out[c] = acc;
  }
}

// K1 for GaussianProcessPriorPose3 (GaussianProcessPriorPose3.h:60-98), whitened rows straight into the row table.
// The 12 x 24 Jacobian is never held as a whole: with Jinv = Jr^-1(r), FD = d(Jinv v2)/dr, the right half
// [H3 H4] = [[Jinv, 0], [FD Jinv, Jinv]] is whitened and stored first, then the left half
// [H1 H2] = [[J, -dt I], [FD J, -I]], J = -Jinv Ad(h^-1); whitening R = [[sa U, sb U], [0, sc U]] is applied as
// U x (block lower-triangular) products row by row, skipping the structural zeros.  Peak live state is FD + two
// 6x6 blocks instead of two 6 x 24 arrays, which is what lets two waves share a SIMD.
// K1 for a chain whose GP priors reach the fused level-0 kernel as structured records (kGps* above): Log, Jr^-1, the
// finite-difference block and J = -Jr^-1 Ad(h^-1) per factor, the whitened error -- and none of the products that turn them
// into Jacobian columns (those moved to the consumer, where they are DPP row operations).
#ifdef GPS_TRACE_KLIN
// debug builds only (scripts/trace_klin.py): s_memrealtime stamps of the K1 waves -- 16 per wave, wave = f / 64
static __device__ unsigned long long g_klin_trace[4096 * 16];
#define KL_TR(slot) do { if (lane == 0 && (f >> 6) < 4096) g_klin_trace[(size_t)(f >> 6) * 16 + (slot)] = wall_clock64(); } while (0)
#else
#define KL_TR(slot) do { } while (0)
#endif
template <typename T>
__device__ __forceinline__ void gp_pose3_record(const GpArgs<T> &a, bool valid, int f, T *st, int *sr, int lane, T &err) {
  KL_TR(0);
  T *mine = st + lane * 20;
  sr[lane] = valid ? f : -1;                 // structured records are indexed by factor, not by row
  const T *U = a.U.u;
  T p1[12], p2[12], v1[6], v2[6];
  T dt = T(1);
#pragma unroll
  for (int k = 0; k < 12; k++) { p1[k] = (k == 0 || k == 4 || k == 8) ? T(1) : T(0); p2[k] = p1[k]; }   // idle lane: identity
#pragma unroll
  for (int k = 0; k < 6; k++) { v1[k] = T(0); v2[k] = T(0); }
  if (valid) {
    const int i = a.left[f];
    dt = a.dt[f];
    if constexpr (std::is_same<T, double>::value) {
      // (with an update pending this thread owns state i, and the chain's last state if that is its right one)
      load_two_states_upd<POSE3>(a.pose, a.vel, a.stride, i, a.pend, true, i + 1 == a.pend.last, p1, v1, p2, v2);
    } else {
#pragma unroll
      for (int k = 0; k < 12; k++) { p1[k] = T(a.pose[(size_t)k * a.stride + i]); p2[k] = T(a.pose[(size_t)k * a.stride + i + 1]); }
#pragma unroll
      for (int k = 0; k < 6; k++) { v1[k] = a.vel[(size_t)k * a.stride + i]; v2[k] = a.vel[(size_t)k * a.stride + i + 1]; }
    }
  }
  KL_TR(1);
  const SE3<T> h = se3_between(as_se3(p1), as_se3(p2));
  const V6<T> r = se3_log(h);                 // GaussianProcessPriorPose3.h:72
#ifdef GPS_TRACE_KLIN
  { V6<T> rr_ = r; pin(rr_); }
  KL_TR(2);
#endif
  const JrK<T> k0 = jr_coefs(r.w);
  const BL6<T> Jinv = se3_jrinv_k(k0, r);     // :76
  const V6<T> u1 = as_v6(v1), u2 = as_v6(v2);
  const T sq = sqrt(dt);
  const T sa = T(3.4641016151377545870548926830117) / (dt * sq);  // sqrt(12 / dt^3)
  const T sb = T(-1.7320508075688772935274463415059) / sq;        // (-6 / dt^2) / sa
  const T sc = T(1) / sq;                                          // sqrt(4/dt - sb^2)
  {   // the whitened error and the scalars: line 4 of the record
    const V6<T> top = r - dt * u1;            // :97
    const V6<T> bot = Jinv * u2 - u1;
    const T e[12] = {top.w.x, top.w.y, top.w.z, top.v.x, top.v.y, top.v.z, bot.w.x, bot.w.y, bot.w.z, bot.v.x, bot.v.y, bot.v.z};
#pragma unroll
    for (int rho = 0; rho < 6; rho++) {
      T wt = T(0), wb = T(0);
#pragma unroll
      for (int q = rho; q < 6; q++) {
        wt += U[rho * 6 + q] * (sa * e[q] + sb * e[6 + q]);
        wb += U[rho * 6 + q] * e[6 + q];
      }
      wb *= sc;
      err += wt * wt + wb * wb;
      mine[rho] = wt;
      mine[6 + rho] = wb;
    }
    mine[12] = -(sa * dt + sb); mine[13] = sb; mine[14] = sc; mine[15] = sa;
    KL_TR(3);
    wave_store_part<T, kGpsLen, 16, 20, true>(st, sr, lane, 0, kGpsE, a.gps);
    KL_TR(4);
  }
  // the matrix blocks in record order, 16 doubles (one 128-byte line) staged per lane at a time
  auto put = [&](int idx, T v) {              // (idx is a compile-time constant once the loops below are unrolled)
    mine[idx & 15] = v;
    if ((idx & 15) == 15) wave_store_part<T, kGpsLen, 16, 20, true>(st, sr, lane, 0, idx - 15, a.gps);
  };
#pragma unroll
  for (int k = 0; k < 9; k++) put(kGpsXA + k, Jinv.A.m[k]);
#pragma unroll
  for (int k = 0; k < 9; k++) put(kGpsXC + k, Jinv.C.m[k]);
  {
    const SE3<T> hi = se3_inverse(h);
    // J = -Jinv Ad(h^-1), Ad = [[R, 0], [t^ R, R]]: the diagonal blocks of J are equal (those of both factors are)
    const M3<T> JA = neg(Jinv.A * hi.R);
    const M3<T> JC = neg(Jinv.C * hi.R + Jinv.A * (skew(hi.t) * hi.R));
#pragma unroll
    for (int k = 0; k < 9; k++) put(kGpsJA + k, JA.m[k]);
#pragma unroll
    for (int k = 0; k < 9; k++) put(kGpsJC + k, JC.m[k]);
  }
  KL_TR(5);
  {   // last, with nothing but r, the coefficients and v2 alive next to it: the twelve evaluations of the difference quotient
    // (the factor's error sum waits in a spare staging slot of the lane: across this block it was what the allocator spilled)
    mine[16] = err;
    BL6<T> FD = se3_jrinv_times_x_fd_k(k0, r, u2);   // (:81, :90)
#ifdef GPS_TRACE_KLIN
    pin(FD.A); pin(FD.C); pin(FD.D);
    KL_TR(6);
#endif
#pragma unroll
    for (int k = 0; k < 9; k++) put(kGpsFA + k, FD.A.m[k]);
#pragma unroll
    for (int k = 0; k < 9; k++) put(kGpsFC + k, FD.C.m[k]);
#pragma unroll
    for (int k = 0; k < 9; k++) put(kGpsFD + k, FD.D.m[k]);
    put(kGpsZ, T(0));
    err = mine[16];
  }
  KL_TR(7);
}

template <typename T, bool VW>
__device__ __forceinline__ void gp_pose3_rows(const GpArgs<T> &a, bool valid, int f, T *st, int *sr, int lane, T &err) {
  constexpr int LS = 14;
  T *mine = st + lane * LS;
  const T *U = a.U.u;
  T p1[12], p2[12], v1[6], v2[6];
  T dt = T(1);
#pragma unroll
  for (int k = 0; k < 12; k++) { p1[k] = (k == 0 || k == 4 || k == 8) ? T(1) : T(0); p2[k] = p1[k]; }   // idle lane: identity
#pragma unroll
  for (int k = 0; k < 6; k++) { v1[k] = T(0); v2[k] = T(0); }
  if (valid) {
    const int i = a.left[f];
    dt = a.dt[f];
    double q1[12], q2[12];
#pragma unroll
    for (int k = 0; k < 12; k++) { q1[k] = a.pose[(size_t)k * a.stride + i]; q2[k] = a.pose[(size_t)k * a.stride + i + 1]; }
    if (!IsF64<T>::v) {
#pragma unroll
      for (int k = 9; k < 12; k++) { q2[k] -= q1[k]; q1[k] = 0.0; }
    }
#pragma unroll
    for (int k = 0; k < 12; k++) { p1[k] = T(q1[k]); p2[k] = T(q2[k]); }
#pragma unroll
    for (int k = 0; k < 6; k++) { v1[k] = a.vel[(size_t)k * a.stride + i]; v2[k] = a.vel[(size_t)k * a.stride + i + 1]; }
  }
  if (VW) {   // GaussianProcessPriorPose3VW.h:87-88: body velocities of the world-frame (v, w)
    T b1[6], b2[6];
    vw_to_vb(p1, v1, b1);
    vw_to_vb(p2, v2, b2);
#pragma unroll
    for (int k = 0; k < 6; k++) { v1[k] = b1[k]; v2[k] = b2[k]; }
  }
  const SE3<T> h = se3_between(as_se3(p1), as_se3(p2));
  const V6<T> r = se3_log(h);                 // GaussianProcessPriorPose3.h:72
  const JrK<T> k0 = jr_coefs(r.w);
  const BL6<T> Jinv = se3_jrinv_k(k0, r);     // :76
  const V6<T> u1 = as_v6(v1), u2 = as_v6(v2);
  const T sq = sqrt(dt);
  const T sa = T(3.4641016151377545870548926830117) / (dt * sq);  // sqrt(12 / dt^3)
  const T sb = T(-1.7320508075688772935274463415059) / sq;        // (-6 / dt^2) / sa
  const T sc = T(1) / sq;                                          // sqrt(4/dt - sb^2)
  {
    const V6<T> top = r - dt * u1;            // :97
    const V6<T> bot = Jinv * u2 - u1;
    const T e[12] = {top.w.x, top.w.y, top.w.z, top.v.x, top.v.y, top.v.z, bot.w.x, bot.w.y, bot.w.z, bot.v.x, bot.v.y, bot.v.z};
#pragma unroll
    for (int rho = 0; rho < 6; rho++) {
      T wt = T(0), wb = T(0);
#pragma unroll
      for (int q = rho; q < 6; q++) {
        wt += U[rho * 6 + q] * (sa * e[q] + sb * e[6 + q]);
        wb += U[rho * 6 + q] * e[6 + q];
      }
      wb *= sc;
      err += wt * wt + wb * wb;
      mine[rho] = wt;
      mine[6 + rho] = wb;
    }
    wave_store_scalars<T, 12>(st, sr, lane, a.rowE);
  }
  const BL6<T> FD = se3_jrinv_times_x_fd_k(k0, r, u2);   // (:81, :90) -- computed once, used twice
  {   // right state: H3 = [Jinv; FD Jinv] (:88-93), H4 = [0; Jinv] (:95)
    const BL6<T> P3 = FD * Jinv;
#pragma unroll
    for (int rho = 0; rho < 6; rho++) {
      T x[6], y[6];
      utri_times_bl6_row(U, Jinv, rho, x);
      utri_times_bl6_row(U, P3, rho, y);
#pragma unroll
      for (int c = 0; c < 6; c++) { mine[c] = sa * x[c] + sb * y[c]; mine[6 + c] = sb * x[c]; }
      if (VW) vw_row_transform(p2, v2, mine);
      wave_store_part<T, 24, 12>(st, sr, lane, rho, 12, a.rowLR);
#pragma unroll
      for (int c = 0; c < 6; c++) { mine[c] = sc * y[c]; mine[6 + c] = sc * x[c]; }
      if (VW) vw_row_transform(p2, v2, mine);
      wave_store_part<T, 24, 12>(st, sr, lane, 6 + rho, 12, a.rowLR);
    }
  }
  {   // left state: H1 = [J; FD J], J = Hlog Hcomp1 Hinv = -Jinv Ad(h^-1) (:79-84), H2 = [-dt I; -I] (:86)
    const BL6<T> J = neg(Jinv * se3_adjoint(se3_inverse(h)));
    const BL6<T> P1 = FD * J;
    const T k2 = -(sa * dt + sb);
#pragma unroll
    for (int rho = 0; rho < 6; rho++) {
      T x[6], y[6];
      utri_times_bl6_row(U, J, rho, x);
      utri_times_bl6_row(U, P1, rho, y);
#pragma unroll
      for (int c = 0; c < 6; c++) { mine[c] = sa * x[c] + sb * y[c]; mine[6 + c] = (c >= rho) ? k2 * U[rho * 6 + c] : T(0); }
      if (VW) vw_row_transform(p1, v1, mine);
      wave_store_part<T, 24, 12>(st, sr, lane, rho, 0, a.rowLR);
#pragma unroll
      for (int c = 0; c < 6; c++) { mine[c] = sc * y[c]; mine[6 + c] = (c >= rho) ? -sc * U[rho * 6 + c] : T(0); }
      if (VW) vw_row_transform(p1, v1, mine);
      wave_store_part<T, 24, 12>(st, sr, lane, 6 + rho, 0, a.rowLR);
    }
  }
}

// One 128-thread block of GP-prior factors; bid = block index among the GP blocks.  stage / srow: the block's LDS staging
// area (2 * 64 * (2b + 2) elements of T and 128 ints when MODE == 0), owned by the calling kernel so that k_lin can share
// one area between its factor types.
// REC (Pose3 body-velocity chains, fp64, MODE 0): structured records for k_fused_level0 (a.gps) instead of rows -- a template
// parameter, not a run-time branch: the two bodies in one kernel cost both their register budget (256 VGPRs + 368 B of scratch)
template <typename T, int MF, int MODE, bool VW, bool REC = false>
__device__ __forceinline__ void gp_block(const GpArgs<T> &a, const int bid, T *stage, int *srow) {
  static_assert(!REC || (MODE == 0 && !VW && IsF64<T>::v && (MF == POSE3 || MF == POSE2 || MF == ROT3 || MF == LINEAR3)),
                "structured GP records: fp64, SE(3) body-velocity chains and the d = 3 manifolds");
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, b = 2 * d;
  constexpr bool JAC = (MODE != 1);
  constexpr int LS = 2 * b + 2;                       // staging stride (16-byte aligned, conflict-free for b128)
  const int f = bid * 128 + threadIdx.x;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool valid = f < a.count;
  T err = T(0);
  if constexpr (MF == POSE3 && MODE == 0) {
    srow[threadIdx.x] = valid ? a.row0[f] : -1;
    if constexpr (REC) gp_pose3_record<T>(a, valid, f, stage + wv * 64 * 20 /* 16 staged doubles per lane, stride 20 */, srow + wv * 64, lane, err);
    else gp_pose3_rows<T, VW>(a, valid, f, stage + wv * 64 * 20 /* half rows: 14 per lane */, srow + wv * 64, lane, err);
    const T tot = block_sum(T(0.5) * err);
    if (threadIdx.x == 0) a.partial[bid] = tot;
    return;
  }
  T e[b];
  T Jt[JAC ? d * 2 * b : 1], Jb[JAC ? d * 2 * b : 1];
  T dt = T(1);
  if (valid) {
    const int i = a.left[f];
    dt = a.dt[f];
    T p1[pd], p2[pd], v1[d], v2[d];
    if constexpr (REC && d == 3 && IsF64<T>::v) {
      // the d = 3 record launches inside run_gn: the states as the pending update leaves them (PendUpd; nothing pending: as stored);
      // this factor owns its left state, the last factor the chain's last state as well
      double q1[pd], q2[pd], w1[d], w2[d];
      load_two_states_upd<MF>(a.pose, a.vel, a.stride, i, a.pend, true, i + 1 == a.pend.last, q1, w1, q2, w2);
#pragma unroll
      for (int k = 0; k < pd; k++) { p1[k] = T(q1[k]); p2[k] = T(q2[k]); }
#pragma unroll
      for (int k = 0; k < d; k++) { v1[k] = T(w1[k]); v2[k] = T(w2[k]); }
    } else {
    {
      double q1[pd], q2[pd];
#pragma unroll
      for (int k = 0; k < pd; k++) { q1[k] = a.pose[(size_t)k * a.stride + i]; q2[k] = a.pose[(size_t)k * a.stride + i + 1]; }
      if (!IsF64<T>::v) {
#pragma unroll
        for (int k = TransPart<MF>::off; k < TransPart<MF>::off + TransPart<MF>::n; k++) { q2[k] -= q1[k]; q1[k] = 0.0; }
      }
#pragma unroll
      for (int k = 0; k < pd; k++) { p1[k] = T(q1[k]); p2[k] = T(q2[k]); }
    }
#pragma unroll
    for (int k = 0; k < d; k++) { v1[k] = a.vel[(size_t)k * a.stride + i]; v2[k] = a.vel[(size_t)k * a.stride + i + 1]; }
    }
    if constexpr (MF == POSE3) {
      if (a.vw) {
        T b1[6], b2[6];
        vw_to_vb(p1, v1, b1);
        vw_to_vb(p2, v2, b2);
#pragma unroll
        for (int k = 0; k < 6; k++) { v1[k] = b1[k]; v2[k] = b2[k]; }
      }
    }
    GpPrior<T, MF, JAC>::eval(p1, v1, p2, v2, dt, e, Jt, Jb);
    if constexpr (MF == POSE3 && JAC) {
      if (a.vw) {
#pragma unroll
        for (int r = 0; r < d; r++) {
          vw_row_transform(p1, v1, Jt + r * 2 * b); vw_row_transform(p2, v2, Jt + r * 2 * b + b);
          vw_row_transform(p1, v1, Jb + r * 2 * b); vw_row_transform(p2, v2, Jb + r * 2 * b + b);
        }
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < b; k++) e[k] = T(0);
    if (JAC) {
#pragma unroll
      for (int k = 0; k < d * 2 * b; k++) { Jt[k] = T(0); Jb[k] = T(0); }
    }
  }
  if (MODE == 2) {
    if (valid) {
#pragma unroll
      for (int k = 0; k < b; k++) a.out_e[(size_t)f * b + k] = e[k];
      if (a.out_H) {
        T *H = a.out_H + (size_t)f * 4 * b * d;
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
          for (int r = 0; r < d; r++)
#pragma unroll
            for (int c = 0; c < d; c++) {
              H[(q * b + r) * d + c] = Jt[r * 2 * b + q * d + c];
              H[(q * b + d + r) * d + c] = Jb[r * 2 * b + q * d + c];
            }
      }
    }
  } else {
    // whitening R = chol_upper(Q^-1(dt)) = [[sa, sb], [0, sc]] (x) U, U = chol_upper(Qc^-1)
    // (noiseModel::Gaussian::Covariance(calcQ(Qc, dt)), GaussianProcessPriorPose3.h:46)
    const T sq = sqrt(dt);
    const T sa = T(3.4641016151377545870548926830117) / (dt * sq);  // sqrt(12 / dt^3)
    const T sb = T(-1.7320508075688772935274463415059) / sq;        // (-6 / dt^2) / sa
    const T sc = T(1) / sq;                                          // sqrt(4/dt - sb^2)
    if constexpr (REC && d == 3) {
      // the d = 3 record (kGp3*): 16 doubles staged per lane at a time (stride 20), whole 128-byte lines out
      T *st = stage + wv * 64 * 20, *mine = st + lane * 20;
      int *sr = srow + wv * 64;
      sr[lane] = valid ? f : -1;
      auto put = [&](int idx, T v) {            // (idx: a compile-time constant once the loops are unrolled)
        mine[idx & 15] = v;
        if ((idx & 15) == 15) wave_store_part<T, kGp3Len, 16, 20, true>(st, sr, lane, 0, idx - 15, a.gps);
      };
#pragma unroll
      for (int blk = 0; blk < 2; blk++)         // A1 = U (sa J1 + sb .): columns 0..2 of the top rows; A3: columns 6..8
#pragma unroll
        for (int rho = 0; rho < 3; rho++)
#pragma unroll
          for (int c = 0; c < 3; c++) {
            T v = T(0);
#pragma unroll
            for (int r = rho; r < 3; r++) v += a.U.u[rho * 3 + r] * (sa * Jt[r * 12 + 6 * blk + c] + sb * Jb[r * 12 + 6 * blk + c]);
            put((blk ? kGp3A3 : kGp3A1) + rho * 3 + c, v);
          }
#pragma unroll
      for (int rho = 0; rho < 3; rho++) {
        T wt = T(0), wb = T(0);
#pragma unroll
        for (int r = rho; r < 3; r++) {
          wt += a.U.u[rho * 3 + r] * (sa * e[r] + sb * e[3 + r]);
          wb += a.U.u[rho * 3 + r] * e[3 + r];
        }
        wb *= sc;
        err += wt * wt + wb * wb;
        put(kGp3E + rho, wt);
        put(kGp3E + 3 + rho, wb);               // (positions 21..23 of the record: written out of order, both inside the second line)
      }
      put(kGp3S + 0, sa * Jt[3] + sb * Jb[3]);  // kLt: the (0, 0) entry of H2's halves
      put(kGp3S + 1, sa * Jt[9] + sb * Jb[9]);  // kRt: H4's
      put(kGp3S + 2, sc * Jb[3]);               // kLb
      put(kGp3S + 3, sc * Jb[9]);               // kRb
      put(28, T(0)); put(29, T(0)); put(30, T(0));
      put(31, T(0));
      const T tot = block_sum(T(0.5) * err);
      if (threadIdx.x == 0) a.partial[bid] = tot;
      return;
    }
    T *st = stage + (MODE == 0 ? wv * 64 * LS : 0);
    T *mine = st + (MODE == 0 ? lane * LS : 0);
    const int *sr = srow + (MODE == 0 ? wv * 64 : 0);
    int row0 = 0;
    if (MODE == 0) {
      row0 = valid ? a.row0[f] : -1;
      srow[threadIdx.x] = row0;
    }
    if (MODE == 1 && a.rowE32 && valid) row0 = a.row0[f];
#pragma unroll
    for (int rho = 0; rho < d; rho++) {
      T wt = T(0), wb = T(0);
#pragma unroll
      for (int r = rho; r < d; r++) {
        wt += a.U.u[rho * d + r] * (sa * e[r] + sb * e[d + r]);
        wb += a.U.u[rho * d + r] * e[d + r];
      }
      wb *= sc;
      err += wt * wt + wb * wb;
      if (MODE == 1 && a.rowE32 && valid) {
        a.rowE32[row0 + rho] = (float)wt;
        a.rowE32[row0 + d + rho] = (float)wb;
      }
      if (MODE == 0) {
        if (valid) {
          a.rowE[row0 + rho] = wt;
          a.rowE[row0 + d + rho] = wb;
        }
#pragma unroll
        for (int col = 0; col < 2 * b; col++) {
          T vt = T(0);
#pragma unroll
          for (int r = rho; r < d; r++) vt += a.U.u[rho * d + r] * (sa * Jt[r * 2 * b + col] + sb * Jb[r * 2 * b + col]);
          mine[col] = vt;
        }
        wave_store_rows<T, 2 * b>(st, sr, lane, rho, a.rowLR);
#pragma unroll
        for (int col = 0; col < 2 * b; col++) {
          T vb = T(0);
#pragma unroll
          for (int r = rho; r < d; r++) vb += a.U.u[rho * d + r] * Jb[r * 2 * b + col];
          mine[col] = sc * vb;
        }
        wave_store_rows<T, 2 * b>(st, sr, lane, d + rho, a.rowLR);
      }
    }
  }
  if (MODE != 2) {
    const T tot = block_sum(T(0.5) * err);
    if (threadIdx.x == 0) a.partial[bid] = tot;
  }
}

// MODE 0: whitened rows + error; MODE 1: error only; MODE 2: unwhitened e + H1..H4 in API layout
template <typename T, int MF, int MODE, bool VW = false, bool REC = false>
__global__ void __launch_bounds__(128) k_gp(GpArgs<T> a) {
  constexpr int LS = REC ? 20 : 4 * MTraits<MF>::d + 2;
  __shared__ T stage[MODE == 0 ? 2 * 64 * LS : 1];
  __shared__ int srow[MODE == 0 ? 128 : 1];
  gp_block<T, MF, MODE, VW, REC>(a, blockIdx.x, stage, srow);
}

// ------------------------------------------------------------------ unary / between rows

template <typename T> struct FacArgs {
  PendUpd pend;         // see GpArgs: these factors read the updated states too (they own none)
  const double *pose, *vel;
  int stride, count, chart;
  const int *idx;       // state (left state for between)
  const double *meas;   // count x (pd or d)
  const double *sig;    // count x d
  const int *row0;
  float *rowE32;        // error-only pass: fp32 copy of the whitened error (fp32 mode), or null
  T *rowLR, *rowE;
  T *partial;
  T *rec;               // KIND 2, Pose3, fp64: structured records (kBtw*) instead of compact rows, or null
};

// BetweenFactor<Pose3> as a structured record (kBtw*): the block-triangular halves of H1 and H2, the weights, the whitened error
template <typename T>
__device__ __forceinline__ void between_pose3_record(const FacArgs<T> &a, const int bid, T *stage, int *srow) {
  const int f = bid * 128 + threadIdx.x;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool valid = f < a.count;
  T *st = stage + wv * 64 * 20, *mine = st + lane * 20;
  int *sr = srow + wv * 64;
  sr[lane] = valid ? f : -1;
  T x1[12], x2[12], m[12];
#pragma unroll
  for (int k = 0; k < 12; k++) { x1[k] = (k == 0 || k == 4 || k == 8) ? T(1) : T(0); x2[k] = x1[k]; m[k] = x1[k]; }   // idle lane: identities
  if (valid) {
    const int i = a.idx[f];
    if constexpr (std::is_same<T, double>::value) {
      double vv[6];
      double vv2[6];
      load_two_states_upd<POSE3>(a.pose, a.vel, a.stride, i, a.pend, false, false, x1, vv, x2, vv2);
#pragma unroll
      for (int k = 0; k < 12; k++) m[k] = T(a.meas[(size_t)f * 12 + k]);
    } else {
#pragma unroll
      for (int k = 0; k < 12; k++) {
        x1[k] = T(a.pose[(size_t)k * a.stride + i]);
        x2[k] = T(a.pose[(size_t)k * a.stride + i + 1]);
        m[k] = T(a.meas[(size_t)f * 12 + k]);
      }
    }
  }
  auto put = [&](int idx, T v) {              // (idx: a compile-time constant once the loops are unrolled)
    mine[idx & 15] = v;
    if ((idx & 15) == 15) wave_store_part<T, kBtwLen, 16, 20, true>(st, sr, lane, 0, idx - 15, a.rec);
  };
  const SE3<T> hx = se3_between(as_se3(x1), as_se3(x2));
  const V6<T> xi = se3_log(se3_between(as_se3(m), hx));          // PoseFactors<T, POSE3>::between
  const BL6<T> HL = se3_jrinv(xi);
#pragma unroll
  for (int k = 0; k < 9; k++) put(kBtwRA + k, HL.A.m[k]);
#pragma unroll
  for (int k = 0; k < 9; k++) put(kBtwRC + k, HL.C.m[k]);
  {
    const SE3<T> hi = se3_inverse(hx);
    const M3<T> LA = neg(HL.A * hi.R);
    const M3<T> LC = neg(HL.C * hi.R + HL.A * (skew(hi.t) * hi.R));
#pragma unroll
    for (int k = 0; k < 9; k++) put(kBtwLA + k, LA.m[k]);
#pragma unroll
    for (int k = 0; k < 9; k++) put(kBtwLC + k, LC.m[k]);
  }
  const T e[6] = {xi.w.x, xi.w.y, xi.w.z, xi.v.x, xi.v.y, xi.v.z};
  T err = T(0), we[6];
#pragma unroll
  for (int r = 0; r < 6; r++) {
    const T w = valid ? T(1) / T(a.sig[(size_t)f * 6 + r]) : T(0);
    we[r] = e[r] * w;
    err += we[r] * we[r];
    put(kBtwW + r, w);
  }
#pragma unroll
  for (int r = 0; r < 6; r++) put(kBtwE + r, we[r]);
  const T tot = block_sum(T(0.5) * err);
  if (threadIdx.x == 0) a.partial[bid] = tot;
}

// KIND 0: PriorFactor<Pose>, 1: PriorFactor<Vector> on the velocity, 2: BetweenFactor<Pose>(x_i, x_i+1)
template <typename T, int MF, int KIND, bool JAC>
__device__ __forceinline__ void simple_block(const FacArgs<T> &a, const int bid, T *stage, int *srow) {
  if constexpr (KIND == 2 && MF == POSE3 && JAC && IsF64<T>::v) {
    if (a.rec != nullptr) { between_pose3_record<T>(a, bid, stage, srow); return; }
  }
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, b = 2 * d;
  // PriorFactor<Pose> and BetweenFactor<Pose> have no velocity columns: they go to the compact row table,
  // [d/dpose_left (d) | d/dpose_right (d)] per row, which halves what K3 has to read for them
  constexpr int W = (KIND == 1) ? 2 * b : 2 * d;
  constexpr int LS = W + 2;
  const int f = bid * 128 + threadIdx.x;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool valid = f < a.count;
  T err = T(0);
  T e[d], H1[JAC ? d * d : 1], H2[JAC ? d * d : 1];
#pragma unroll
  for (int k = 0; k < d; k++) e[k] = T(0);
  if (JAC) {
#pragma unroll
    for (int k = 0; k < d * d; k++) { H1[k] = T(0); H2[k] = T(0); }
  }
  if (valid) {
    const int i = a.idx[f];
    if (KIND == 1) {
      double pp[pd], vv[d];
      load_state_upd<MF>(a.pose, a.vel, a.stride, i, a.pend, false, pp, vv);
#pragma unroll
      for (int k = 0; k < d; k++) e[k] = T(vv[k] - a.meas[(size_t)f * d + k]);
    } else {
      T x1[pd], m[pd], x2[pd];
      {
        double q1[pd], qm[pd], q2[pd], vv[d];
        load_state_upd<MF>(a.pose, a.vel, a.stride, i, a.pend, false, q1, vv);
        if (KIND == 2) load_state_upd<MF>(a.pose, a.vel, a.stride, i + 1, a.pend, false, q2, vv);
#pragma unroll
        for (int k = 0; k < pd; k++) {
          qm[k] = a.meas[(size_t)f * pd + k];
          if (KIND != 2) q2[k] = 0.0;
        }
        if (!IsF64<T>::v) {   // re-centre on x1: PriorFactor compares (prior, x1), BetweenFactor (x1, x2) with a relative measurement
#pragma unroll
          for (int k = TransPart<MF>::off; k < TransPart<MF>::off + TransPart<MF>::n; k++) {
            if (KIND == 0) qm[k] -= q1[k]; else q2[k] -= q1[k];
            q1[k] = 0.0;
          }
        }
#pragma unroll
        for (int k = 0; k < pd; k++) { x1[k] = T(q1[k]); m[k] = T(qm[k]); x2[k] = T(q2[k]); }
      }
      if (KIND == 0) {
        PoseFactors<T, MF, JAC>::prior(m, x1, a.chart, e, H1);
      } else {
        PoseFactors<T, MF, JAC>::between(m, x1, x2, a.chart, e, H1, H2);
      }
    }
  }
  const int row0 = ((JAC || a.rowE32) && valid) ? a.row0[f] : -1;
  T *st = stage + (JAC ? wv * 64 * LS : 0);
  T *mine = st + (JAC ? lane * LS : 0);
  if (JAC) srow[threadIdx.x] = row0;
#pragma unroll
  for (int r = 0; r < d; r++) {
    const T w = valid ? T(1) / T(a.sig[(size_t)f * d + r]) : T(0);
    const T we = e[r] * w;
    err += we * we;
    if (!JAC && a.rowE32 && valid) a.rowE32[row0 + r] = (float)we;
    if (JAC) {
      if (valid) a.rowE[row0 + r] = we;
#pragma unroll
      for (int c = 0; c < W; c++) mine[c] = T(0);
      if (KIND == 1) {
        mine[d + r] = w;
      } else {
#pragma unroll
        for (int c = 0; c < d; c++) mine[c] = w * H1[r * d + c];
        if (KIND == 2) {
#pragma unroll
          for (int c = 0; c < d; c++) mine[d + c] = w * H2[r * d + c];
        }
      }
      wave_store_rows<T, W>(st, srow + wv * 64, lane, r, a.rowLR);
    }
  }
  const T tot = block_sum(T(0.5) * err);
  if (threadIdx.x == 0) a.partial[bid] = tot;
}

template <typename T, int MF, int KIND, bool JAC>
__global__ void __launch_bounds__(128) k_simple(FacArgs<T> a) {
  constexpr int LS = ((KIND == 1) ? 4 * MTraits<MF>::d : 2 * MTraits<MF>::d) + 2;
  __shared__ T stage[JAC ? 2 * 64 * LS : 1];
  __shared__ int srow[JAC ? 128 : 1];
  simple_block<T, MF, KIND, JAC>(a, blockIdx.x, stage, srow);
}

// K1 of a Gauss-Newton iteration in ONE launch: the GP priors, the pose / velocity priors and the between factors share the
// grid, the register-heavy GP blocks first and the light streaming blocks behind them, which fill the issue slots and the
// store bandwidth the GP waves leave (measured on 1e5 Pose3 states: 0.539 ms per iteration; the same kernels on two streams
// with an event fork / join 0.556; GP and between blocks alternating 0.568).
template <typename T> struct LinArgs {
  GpArgs<T> gp;
  FacArgs<T> fac[3];      // pose priors, velocity priors, between factors
  int nb_gp, nb[3];       // blocks per type (0: type absent)
  // deferred reduction (round 3): the per-block |delta|_inf maxima the PREVIOUS iteration's k_retract left behind are
  // reduced here, by one extra workgroup at the end of the grid, instead of by a launch of their own (fixed order:
  // deterministic; nothing is skipped, the value lands in *red_out one launch later).  red_in == null: nothing pending.
  const double *red_in = nullptr;
  int red_n = 0;
  double *red_out = nullptr;
};
// VP: the launch contains velocity priors (full-width rows).  Without them a Pose3 launch stages half rows only (the GP
// prior writes its rows in halves, pose priors / between factors have compact rows): 14 KB of LDS instead of 27 KB, so that
// every workgroup of a 1e5-state launch is resident at once.
template <typename T, int MF, bool VW, bool VP, bool REC = false>
__global__ void __launch_bounds__(128, kLinWaves) k_lin(LinArgs<T> a) {
  constexpr int LS = (MF == POSE3 && !VP) ? 20 : (4 * MTraits<MF>::d + 2 > 20 || !REC ? 4 * MTraits<MF>::d + 2 : 20);
  __shared__ T stage[2 * 64 * LS];
  __shared__ int srow[128];
  int bid = blockIdx.x;
  if (a.red_in != nullptr && bid == (int)gridDim.x - 1) {     // the extra workgroup: pending maximum of the previous retraction
    const double acc = strided_fold<double, 128>(a.red_in, a.red_n, 1);
    const double r = block_max(acc);
    if (threadIdx.x == 0) *a.red_out = r;
    return;
  }
  // GP blocks first, then the light ones (measured in round 2: 0.539 ms per iteration; GP and between blocks alternating 0.568)
  if (bid < a.nb_gp) { gp_block<T, MF, 0, VW, REC>(a.gp, bid, stage, srow); return; }
  bid -= a.nb_gp;
  if (bid < a.nb[2]) { simple_block<T, MF, 2, true>(a.fac[2], bid, stage, srow); return; }
  bid -= a.nb[2];
  if (bid < a.nb[0]) { simple_block<T, MF, 0, true>(a.fac[0], bid, stage, srow); return; }
  bid -= a.nb[0];
  if constexpr (VP) simple_block<T, MF, 1, true>(a.fac[1], bid, stage, srow);
}

// ------------------------------------------------------------------ K2: measurement factors

enum FKind : int { FK_INTERP_RANGE = 0, FK_RANGE = 1, FK_INTERP_ATT = 2, FK_INTERP_GPS = 3, FK_ODOM2D = 4, FK_BEARING_RANGE = 5, FK_INTERP_PROJ = 6, FK_AHRS = 7 };
constexpr int kNumMeasKinds = 8;
constexpr int kAhrsWidth = 34;   // per-factor parameters of FK_AHRS: the 25 of ahrs_factor() + sqrt information R (3 x 3, upper triangular)
constexpr int kMeasAux = 22;     // [body_P_sensor (12) | fx, fy, s, u0, v0 | has_sensor | k1, k2, p1, p2 (Cal3DS2; zeros: Cal3_S2)]
template <int FK> struct FKRows { static constexpr int rows = (FK == FK_INTERP_RANGE || FK == FK_RANGE) ? 1 : ((FK == FK_INTERP_ATT || FK == FK_BEARING_RANGE || FK == FK_INTERP_PROJ) ? 2 : 3); };

template <typename T> struct MeasArgs {
  PendUpd pend;        // d = 3 chains inside run_gn: the update k_lin is applying beside this launch (pose / vel: the buffer it READS)
  const double *pose, *vel;
  int stride;
  const double *lmk;   // L x ld (AoS)
  int ld, count, chart;
  const int *idx;      // left (or only) state
  const int *lm;       // landmark or null
  const double *meas;  // count x mw
  int mw;
  const double *sig;   // count x rows
  const double *coef;  // count x 4: l11, l12, p11, p12 (interpolated kinds)
  float *rowE32;       // error-only pass: fp32 copy of the whitened error (fp32 mode), or null
  T *out_e, *out_J;    // inspection (gpslam_hip_linearize_meas): unwhitened e (count x rows) and per row
                       // [H1 H2 | H3 H4 | H5 (3, zero padded)] exactly as evaluateError returns them, or null
  const double *aux;       // table of kMeasAux-wide entries [body_P_sensor (12) | fx, fy, s, u0, v0 | has_sensor | k1, k2, p1, p2]
  const int *aidx;     // count: entry of each factor (one body_P_sensor / calibration PER FACTOR, as in the reference:
                       // GPInterpolatedRangeFactorPose3.h:46-54), or null: no sensor transform anywhere
  const double *sqi;   // count x rows x rows square-root information R (upper triangular, R^T R = cov^-1) of factors with a
                       // noiseModel::Gaussian instead of diagonal sigmas (multi-row kinds; `sig` is then ignored), or null
  int vw;              // Pose3 only: velocities are world-frame [v; w]
  // Pose3, Jacobian pass (round 4): the structured records K1 has just written (kGps*) and the record index per left state (n + 2
  // entries, -1: no GP prior on that interval) -- interp_pose3 takes Jinv, Jinv Ad(h^-1) and the finite-difference block of the
  // interval from there instead of forming them again for every measurement factor on it.  Null: it forms them.
  const T *gps = nullptr;
  const int *gpidx = nullptr;
  T *rowI = nullptr;   // k_gps_lines: the table of 16-double interpolated rows (kIRow*); row0 then counts rows of THAT table
  const int *row0;
  T *rowLR, *rowE, *rowM;
  int *rowLm;
  T *partial;
  // noiseModel::Robust (gpslam_hip_set_meas_robust, robust.hpp): count x 2 = (loss, k) per factor, or null: no factor of this kind
  // carries a loss; out_w (count, or null): every factor's weight w(r), 1 without a loss (gpslam_hip_get_meas_weights)
  const double *rob = nullptr;
  T *out_w = nullptr;
};

// valid (manifold, kind) pairs; everything else is rejected on the host and compiles to an empty kernel
template <int MF, int FK> struct MeasValid {
  static constexpr bool v = ((FK == FK_INTERP_RANGE || FK == FK_RANGE) && (MF == POSE2 || MF == POSE3 || MF == LINEAR3)) ||
                            (FK == FK_INTERP_ATT && (MF == ROT3 || MF == ROT3_BIAS)) || (FK == FK_AHRS && MF == ROT3_BIAS) ||
                            ((FK == FK_INTERP_GPS || FK == FK_INTERP_PROJ) && MF == POSE3) ||
                            ((FK == FK_ODOM2D || FK == FK_BEARING_RANGE) && MF == LINEAR3);
};

template <typename T> __device__ __forceinline__ void put_v3(V3<T> a, T *row) { row[0] = a.x; row[1] = a.y; row[2] = a.z; }
template <typename T> __device__ __forceinline__ void put_v6(V6<T> a, T *row) { put_v3(a.w, row); put_v3(a.v, row + 3); }

// GPInterpolatedRangeFactorPose2/Pose3/2DLinear, RangeFactorPose2 / RangeFactor2DLinear,
// GPInterpolatedAttitudeFactorRot3, GPInterpolatedGPSFactorPose3, OdometryFactor2DLinear, RangeBearingFactor2DLinear
// (gpslam/slam/*.h, see the per-branch citations).  One thread per factor.
// (GPInterpolatedGPSFactorPose3 as 16-double lines for k_fused_level0<4>: k_gps_lines below)
template <typename T, int MF, int FK, bool JAC>
__global__ void __launch_bounds__(128) k_meas(MeasArgs<T> a) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, b = 2 * d, rows = FKRows<FK>::rows;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  T err = T(0);
  if constexpr (MeasValid<MF, FK>::v) {
    // whitened Jacobian rows leave through the per-wave staging buffer (wave_store_rows), like the GP prior's
    T JL[JAC ? rows * b : 1], JR[JAC ? rows * b : 1], wgt[rows];
    int row0v = -1;
#pragma unroll
    for (int r = 0; r < rows; r++) wgt[r] = T(0);
    if (f < a.count) {
      const int i = a.idx[f];
      constexpr bool two = (FK == FK_INTERP_RANGE || FK == FK_INTERP_ATT || FK == FK_INTERP_GPS || FK == FK_ODOM2D || FK == FK_INTERP_PROJ || FK == FK_AHRS);
      constexpr bool haslm = (FK == FK_INTERP_RANGE || FK == FK_RANGE || FK == FK_BEARING_RANGE || FK == FK_INTERP_PROJ);
      T p1[pd], v1[d], p2[pd], v2[d];
      double org[3] = {0.0, 0.0, 0.0};      // fp32 arithmetic: translations re-centred on the first pose (see TransPart)
      // (round 5) the d = 3 chains run this kernel BESIDE k_lin on a second stream: with an update pending (PendUpd) both read the
      // old state buffer and apply the update themselves; k_lin alone writes the other buffer
      constexpr bool PEND = JAC && IsF64<T>::v && two && (MF == POSE2 || MF == ROT3 || MF == LINEAR3);
      if constexpr (PEND) {
        double q1[pd], q2[pd], w1[d], w2[d];
        load_two_states_upd<MF>(a.pose, a.vel, a.stride, i, a.pend, false, false, q1, w1, q2, w2);
#pragma unroll
        for (int k = 0; k < pd; k++) { p1[k] = T(q1[k]); p2[k] = T(q2[k]); }
#pragma unroll
        for (int k = 0; k < d; k++) { v1[k] = T(w1[k]); v2[k] = T(w2[k]); }
      } else {
      {
        double q1[pd], q2[pd];
#pragma unroll
        for (int k = 0; k < pd; k++) { q1[k] = a.pose[(size_t)k * a.stride + i]; q2[k] = two ? a.pose[(size_t)k * a.stride + i + 1] : 0.0; }
        if (!IsF64<T>::v) {
#pragma unroll
          for (int k = 0; k < TransPart<MF>::n; k++) {
            if (k < 3) org[k] = q1[TransPart<MF>::off + k];
            if (two) q2[TransPart<MF>::off + k] -= q1[TransPart<MF>::off + k];
            q1[TransPart<MF>::off + k] = 0.0;
          }
        }
#pragma unroll
        for (int k = 0; k < pd; k++) { p1[k] = T(q1[k]); p2[k] = T(q2[k]); }
      }
#pragma unroll
      for (int k = 0; k < d; k++) { v1[k] = a.vel[(size_t)k * a.stride + i]; v2[k] = two ? a.vel[(size_t)k * a.stride + i + 1] : T(0); }
      }
      if constexpr (MF == POSE3 && two) {
        if (a.vw) {     // GaussianProcessInterpolatorPose3VW.h:79-80
          T b1[6], b2[6];
          vw_to_vb(p1, v1, b1);
          vw_to_vb(p2, v2, b2);
#pragma unroll
          for (int k = 0; k < 6; k++) { v1[k] = b1[k]; v2[k] = b2[k]; }
        }
      }
      int lm = -1;
      T pt[3] = {T(0), T(0), T(0)};
      if (haslm) {
        lm = a.lm[f];
        for (int q = 0; q < a.ld; q++) pt[q] = T(a.lmk[(size_t)lm * a.ld + q] - org[q]);
      }
      const T *gprec = nullptr;      // the interval's GaussianProcessPriorPose3 record, when K1 left one (see MeasArgs::gps)
      if constexpr (MF == POSE3 && JAC && std::is_same<T, double>::value) {
        if (a.gps != nullptr && two) {
          const int g = a.gpidx[i];
          if (g >= 0) gprec = a.gps + (size_t)g * kGpsLen;
        }
      }
      ICoef<T> kc = {T(0), T(0), T(0), T(0)};
      if (FK == FK_INTERP_RANGE || FK == FK_INTERP_ATT || FK == FK_INTERP_GPS || FK == FK_INTERP_PROJ)
        kc = {T(a.coef[4 * (size_t)f]), T(a.coef[4 * (size_t)f + 1]), T(a.coef[4 * (size_t)f + 2]), T(a.coef[4 * (size_t)f + 3])};
      T ms[6];
#pragma unroll
      for (int k = 0; k < 6; k++) ms[k] = (k < a.mw) ? T(a.meas[(size_t)f * a.mw + k]) : T(0);
      // per-factor body_P_sensor / calibration (identical entries are shared through the table)
      const double *ax = a.aidx ? a.aux + (size_t)a.aidx[f] * kMeasAux : nullptr;
      const bool has_sensor = ax && ax[17] != 0.0;
      T sens[12];
#pragma unroll
      for (int k = 0; k < 12; k++) sens[k] = (has_sensor && k < pd) ? T(ax[k]) : T(0);
      T e[rows];
      T Jm[JAC ? rows * 3 : 1];
      if (JAC) {
#pragma unroll
        for (int k = 0; k < rows * b; k++) { JL[k] = T(0); JR[k] = T(0); }
#pragma unroll
        for (int k = 0; k < rows * 3; k++) Jm[k] = T(0);
      }

      if constexpr ((FK == FK_INTERP_RANGE || FK == FK_RANGE) && MF == POSE3) {
        // GPInterpolatedRangeFactorPose3::evaluateError, gpslam/slam/GPInterpolatedRangeFactorPose3.h:64-98
        Interp6Out<T, JAC> o;
        SE3<T> pose = (FK == FK_INTERP_RANGE) ? interp_pose3<T, JAC>(p1, v1, p2, v2, kc, o, gprec) : as_se3(p1);
        const SE3<T> S = as_se3(sens);
        const SE3<T> sp = has_sensor ? se3_compose(pose, S) : pose;
        const V3<T> pw = {pt[0], pt[1], pt[2]};
        const V3<T> q = tmul(sp.R, pw - sp.t);                       // Pose3::transform_to
        const T r = sqrt(dot(q, q));
        const V3<T> qh = (T(1) / r) * q;
        e[0] = r - ms[0];
        if (JAC) {
          V6<T> Hr = {rowmul(qh, skew(q)), -qh};                     // D_r_local * [skew(q), -I]
          if (has_sensor) Hr = rowmul(Hr, se3_adjoint(se3_inverse(S)));   // Hpose * H0 (:87)
          put_v3(sp.R * qh, Jm);                                     // D_r_local * R^T
          if (FK == FK_INTERP_RANGE) {
            put_v6(rowmul(Hr, o.H1), JL); put_v6(rowmul(Hr, o.H2), JL + 6);
            put_v6(rowmul(Hr, o.H3), JR); put_v6(rowmul(Hr, o.H4), JR + 6);
          } else {
            put_v6(Hr, JL);
          }
        }
      } else if constexpr ((FK == FK_INTERP_RANGE || FK == FK_RANGE) && MF == POSE2) {
        // GPInterpolatedRangeFactorPose2::evaluateError, gpslam/slam/GPInterpolatedRangeFactorPose2.h:64-98
        Interp3Out<T, JAC> o;
        SE2<T> pose = (FK == FK_INTERP_RANGE) ? interp_pose2<T, JAC>(p1, v1, p2, v2, kc, o) : SE2<T>{p1[0], p1[1], p1[2]};
        const SE2<T> S = {sens[0], sens[1], sens[2]};
        const SE2<T> sp = has_sensor ? se2_compose(pose, S) : pose;
        const T dx = pt[0] - sp.x, dy = pt[1] - sp.y;
        const T r = sqrt(dx * dx + dy * dy);
        const T hx = dx / r, hy = dy / r;
        e[0] = r - ms[0];
        if (JAC) {
          const T c = cos(sp.th), sn = sin(sp.th);
          V3<T> Hr = {-c * hx - sn * hy, sn * hx - c * hy, T(0)};   // D_r_d * [[-c, s, 0], [-s, -c, 0]]
          if (has_sensor) Hr = rowmul(Hr, se2_adjoint(se2_inverse(S)));
          Jm[0] = hx; Jm[1] = hy;
          if (FK == FK_INTERP_RANGE) {
            put_v3(rowmul(Hr, o.H1), JL); put_v3(rowmul(Hr, o.H2), JL + 3);
            put_v3(rowmul(Hr, o.H3), JR); put_v3(rowmul(Hr, o.H4), JR + 3);
          } else {
            put_v3(Hr, JL);
          }
        }
      } else if constexpr ((FK == FK_INTERP_RANGE || FK == FK_RANGE) && MF == LINEAR3) {
        // GPInterpolatedRangeFactor2DLinear (GPInterpolatedRangeFactor2DLinear.h:60-88) / RangeFactor2DLinear (:43-56)
        T px, py;
        if (FK == FK_INTERP_RANGE) {
          px = kc.l11 * p1[0] + kc.l12 * v1[0] + kc.p11 * p2[0] + kc.p12 * v2[0];
          py = kc.l11 * p1[1] + kc.l12 * v1[1] + kc.p11 * p2[1] + kc.p12 * v2[1];
        } else { px = p1[0]; py = p1[1]; }
        const T dx = pt[0] - px, dy = pt[1] - py;
        const T r = sqrt(dx * dx + dy * dy);
        const T hx = dx / r, hy = dy / r;
        e[0] = r - ms[0];
        if (JAC) {
          Jm[0] = hx; Jm[1] = hy;
          if (FK == FK_INTERP_RANGE) {
            JL[0] = -kc.l11 * hx; JL[1] = -kc.l11 * hy; JL[3] = -kc.l12 * hx; JL[4] = -kc.l12 * hy;
            JR[0] = -kc.p11 * hx; JR[1] = -kc.p11 * hy; JR[3] = -kc.p12 * hx; JR[4] = -kc.p12 * hy;
          } else { JL[0] = -hx; JL[1] = -hy; }
        }
      } else if constexpr (FK == FK_INTERP_ATT) {
        // GPInterpolatedAttitudeFactorRot3::evaluateError, gpslam/slam/GPInterpolatedAttitudeFactorRot3.h:61-83
        Interp3Out<T, JAC> o;
        const M3<T> R = interp_rot3<T, JAC>(p1, v1, p2, v2, kc, o);
        const V3<T> nZ = {ms[0], ms[1], ms[2]}, bRef = {ms[3], ms[4], ms[5]};
        V3<T> q = R * bRef;
        q = (T(1) / sqrt(dot(q, q))) * q;
        V3<T> z1, z2;
        unit3_basis(nZ, z1, z2);
        e[0] = dot(z1, q); e[1] = dot(z2, q);
        if (JAC) {
          V3<T> q1, q2;
          unit3_basis(q, q1, q2);
          const M3<T> RS = R * skew(bRef);
          const V3<T> n1 = -rowmul(q1, RS), n2 = -rowmul(q2, RS);       // D_nRef_R = -Bq^T R [bRef]x
          const T d00 = dot(z1, q1), d01 = dot(z1, q2), d10 = dot(z2, q1), d11 = dot(z2, q2);   // Bz^T Bq
          const V3<T> h0 = d00 * n1 + d01 * n2, h1 = d10 * n1 + d11 * n2;
          // (the velocity columns start at d: 3 for Rot3 states, 6 for the AHRS state whose pose slot also holds the bias)
          put_v3(rowmul(h0, o.H1), JL); put_v3(rowmul(h0, o.H2), JL + d); put_v3(rowmul(h0, o.H3), JR); put_v3(rowmul(h0, o.H4), JR + d);
          put_v3(rowmul(h1, o.H1), JL + b); put_v3(rowmul(h1, o.H2), JL + b + d); put_v3(rowmul(h1, o.H3), JR + b); put_v3(rowmul(h1, o.H4), JR + b + d);
        }
      } else if constexpr (FK == FK_AHRS) {
        // gtsam::AHRSFactor(x_i, x_i+1, b_i, pim) (matlab/GPAHRSexample.m:131-137); noise model = Gaussian with the
        // pre-integrated covariance: the rows are whitened here by its square-root information R (sigmas = 1 below),
        // except in the inspection call, which returns the unwhitened evaluateError() values
        const double *pp = a.meas + (size_t)f * a.mw;
        T prm[25];
#pragma unroll
        for (int k = 0; k < 25; k++) prm[k] = T(pp[k]);
        M3<T> A, B, C;
        ahrs_factor<T, JAC>(as_m3(p1), as_m3(p2), V3<T>{p1[9], p1[10], p1[11]}, prm, e, A, B, C);
        const bool whiten = !(JAC && a.out_e);
        T Rw[9];
#pragma unroll
        for (int k = 0; k < 9; k++) Rw[k] = whiten ? T(pp[25 + k]) : ((k == 0 || k == 4 || k == 8) ? T(1) : T(0));
        const V3<T> ew = as_m3(Rw) * V3<T>{e[0], e[1], e[2]};
        e[0] = ew.x; e[1] = ew.y; e[2] = ew.z;
        if (JAC) {
          put_m3(as_m3(Rw) * A, JL, b, 0, 0);     // d/dx_i
          put_m3(as_m3(Rw) * C, JL, b, 0, 3);     // d/db_i
          put_m3(as_m3(Rw) * B, JR, b, 0, 0);     // d/dx_i+1
        }
      } else if constexpr (FK == FK_INTERP_GPS) {
        // GPInterpolatedGPSFactorPose3::evaluateError, gpslam/slam/GPInterpolatedGPSFactorPose3.h:66-95
        Interp6Out<T, JAC> o;
        const SE3<T> pose = interp_pose3<T, JAC>(p1, v1, p2, v2, kc, o, gprec);
        const SE3<T> S = as_se3(sens);
        const SE3<T> sp = has_sensor ? se3_compose(pose, S) : pose;
        e[0] = sp.t.x - ms[0]; e[1] = sp.t.y - ms[1]; e[2] = sp.t.z - ms[2];
        if (JAC) {
          const BL6<T> AdS = se3_adjoint(se3_inverse(S));
#pragma unroll
          for (int r = 0; r < 3; r++) {
            V6<T> Hp = {{T(0), T(0), T(0)}, {sp.R.m[3 * r], sp.R.m[3 * r + 1], sp.R.m[3 * r + 2]}};   // translation(H) = [0, R]
            if (has_sensor) Hp = rowmul(Hp, AdS);
            put_v6(rowmul(Hp, o.H1), JL + r * b); put_v6(rowmul(Hp, o.H2), JL + r * b + 6);
            put_v6(rowmul(Hp, o.H3), JR + r * b); put_v6(rowmul(Hp, o.H4), JR + r * b + 6);
          }
        }
      } else if constexpr (FK == FK_INTERP_PROJ) {
        // GPInterpolatedProjectionFactorPose3<CALIBRATION>::evaluateError, GPInterpolatedProjectionFactorPose3.h:82-139:
        // PinholeCamera(pose * body_P_sensor, K).project(point); a landmark behind the camera is masked, not thrown
        // (throwCheirality = false): error = 2 fx, all Jacobians zero (:122-138).  CALIBRATION = Cal3_S2, or Cal3DS2 when the
        // entry carries distortion coefficients (radial k1, k2, tangential p1, p2: Cal3DS2_Base::uncalibrate)
        Interp6Out<T, JAC> o;
        const SE3<T> pose = interp_pose3<T, JAC>(p1, v1, p2, v2, kc, o, gprec);
        const SE3<T> S = as_se3(sens);
        const SE3<T> cam = has_sensor ? se3_compose(pose, S) : pose;
        const V3<T> pw = {pt[0], pt[1], pt[2]};
        const V3<T> q = tmul(cam.R, pw - cam.t);
        const T fx = ax ? T(ax[12]) : T(1), fy = ax ? T(ax[13]) : T(1), sk = ax ? T(ax[14]) : T(0), cu0 = ax ? T(ax[15]) : T(0), cv0 = ax ? T(ax[16]) : T(0);
        if (!(q.z > T(0))) {
          e[0] = T(2) * fx; e[1] = T(2) * fx;
        } else {
          const T dz = T(1) / q.z, u = q.x * dz, v = q.y * dz;
          const T k1 = ax ? T(ax[18]) : T(0), k2 = ax ? T(ax[19]) : T(0), t1 = ax ? T(ax[20]) : T(0), t2 = ax ? T(ax[21]) : T(0);
          const T xx = u * u, yy = v * v, xy = u * v, rr = xx + yy;
          const T g = T(1) + k1 * rr + k2 * rr * rr;
          const T pdx = g * u + T(2) * t1 * xy + t2 * (rr + T(2) * xx);     // the distorted intrinsic point (= (u, v) for Cal3_S2)
          const T pdy = g * v + T(2) * t2 * xy + t1 * (rr + T(2) * yy);
          e[0] = fx * pdx + sk * pdy + cu0 - ms[0];
          e[1] = fy * pdy + cv0 - ms[1];
          if (JAC) {
            // PinholeBase::Dpose / Dpoint, then uncalibrate's [[fx, s], [0, fy]] D(pd)/D(pn)
            const T dgx = T(2) * k1 * u + T(4) * k2 * rr * u, dgy = T(2) * k1 * v + T(4) * k2 * rr * v;
            const T d00 = g + u * dgx + T(2) * t1 * v + T(6) * t2 * u, d01 = u * dgy + T(2) * t1 * u + T(2) * t2 * v;
            const T d10 = v * dgx + T(2) * t2 * v + T(2) * t1 * u, d11 = g + v * dgy + T(2) * t2 * u + T(6) * t1 * v;
            const T m00 = fx * d00 + sk * d10, m01 = fx * d01 + sk * d11, m10 = fy * d10, m11 = fy * d11;
            const V6<T> r0 = {{u * v, T(-1) - u * u, v}, {-dz, T(0), dz * u}};
            const V6<T> r1 = {{T(1) + v * v, -u * v, -u}, {T(0), -dz, dz * v}};
            V6<T> h0 = m00 * r0 + m01 * r1, h1 = m10 * r0 + m11 * r1;
            if (has_sensor) {
              const BL6<T> AdS = se3_adjoint(se3_inverse(S));
              h0 = rowmul(h0, AdS);
              h1 = rowmul(h1, AdS);
            }
            const M3<T> &R = cam.R;
            const V3<T> c0 = {R.m[0], R.m[3], R.m[6]}, c1 = {R.m[1], R.m[4], R.m[7]}, c2 = {R.m[2], R.m[5], R.m[8]};
            const V3<T> d0 = dz * (c0 - u * c2), d1 = dz * (c1 - v * c2);
            put_v3(m00 * d0 + m01 * d1, Jm);
            put_v3(m10 * d0 + m11 * d1, Jm + 3);
            put_v6(rowmul(h0, o.H1), JL); put_v6(rowmul(h0, o.H2), JL + 6); put_v6(rowmul(h0, o.H3), JR); put_v6(rowmul(h0, o.H4), JR + 6);
            put_v6(rowmul(h1, o.H1), JL + b); put_v6(rowmul(h1, o.H2), JL + b + 6); put_v6(rowmul(h1, o.H3), JR + b); put_v6(rowmul(h1, o.H4), JR + b + 6);
          }
        }
      } else if constexpr (FK == FK_ODOM2D) {
        // OdometryFactor2DLinear::evaluateError, gpslam/slam/OdometryFactor2DLinear.h:50-75
        const T dx = p2[0] - p1[0], dy = p2[1] - p1[1], dth = p2[2] - p1[2];
        const T c = cos(p1[2]), sn = sin(p1[2]);
        const T qx = c * dx + sn * dy, qy = -sn * dx + c * dy;
        e[0] = qx - ms[0]; e[1] = qy - ms[1]; e[2] = dth - ms[2];
        if (JAC) {
          JL[0] = -c; JL[1] = -sn; JL[2] = qy;
          JL[b + 0] = sn; JL[b + 1] = -c; JL[b + 2] = -qx;
          JL[2 * b + 2] = T(-1);
          JR[0] = c; JR[1] = sn;
          JR[b + 0] = -sn; JR[b + 1] = c;
          JR[2 * b + 2] = T(1);
        }
      } else if constexpr (FK == FK_BEARING_RANGE) {
        // RangeBearingFactor2DLinear::evaluateError, gpslam/slam/RangeBearingFactor2DLinear.h:47-84; meas = (bearing, range)
        const T c = cos(p1[2]), sn = sin(p1[2]);
        const T dx = pt[0] - p1[0], dy = pt[1] - p1[1];
        const T rx = c * dx + sn * dy, ry = -sn * dx + c * dy;           // pose2.transform_to(point)
        const T ed = sqrt(dx * dx + dy * dy);
        const T hx = dx / ed, hy = dy / ed;
        const T df = atan2(ry, rx) - ms[0];
        e[0] = atan2(sin(df), cos(df));
        e[1] = ed - ms[1];
        if (JAC) {
          T t0 = T(0), t1 = T(0);
          if (ed > T(1e-5)) { t0 = -ry / (ed * ed); t1 = rx / (ed * ed); }   // :62
          JL[0] = t0 * (-c) + t1 * sn; JL[1] = t0 * (-sn) + t1 * (-c); JL[2] = t0 * ry + t1 * (-rx);   // tmp * [-R^T, t]
          JL[b + 0] = -hx; JL[b + 1] = -hy;
          Jm[0] = t0 * c + t1 * (-sn); Jm[1] = t0 * sn + t1 * c;       // tmp * R^T
          Jm[3 + 0] = hx; Jm[3 + 1] = hy;
        }
      }

      if constexpr (MF == POSE3 && two && JAC) {
        if (a.vw) {     // chain rule through convertVWtoVb (v1 / v2 hold the body velocities here)
#pragma unroll
          for (int r = 0; r < rows; r++) { vw_row_transform(p1, v1, JL + r * b); vw_row_transform(p2, v2, JR + r * b); }
        }
      }
      if (JAC && a.out_e) {
#pragma unroll
        for (int r = 0; r < rows; r++) {
          a.out_e[(size_t)f * rows + r] = e[r];
          T *o = a.out_J + ((size_t)f * rows + r) * (2 * b + 3);
#pragma unroll
          for (int c = 0; c < b; c++) { o[c] = JL[r * b + c]; o[b + c] = JR[r * b + c]; }
#pragma unroll
          for (int c = 0; c < 3; c++) o[2 * b + c] = Jm[r * 3 + c];
        }
      }
      const int row0 = (JAC || a.rowE32) ? a.row0[f] : 0;
      row0v = row0;
      constexpr bool kFullNoise = rows > 1 && FK != FK_AHRS;     // (AHRSFactor whitens by its pre-integrated covariance above)
      if constexpr (kFullNoise) {
        if (a.sqi) {   // noiseModel::Gaussian: rows <- R rows; R is upper triangular, so ascending in place
          const double *Rw = a.sqi + (size_t)f * rows * rows;
#pragma unroll
          for (int r = 0; r < rows; r++) {
            T acc = T(0);
#pragma unroll
            for (int q = r; q < rows; q++) acc += T(Rw[r * rows + q]) * e[q];
            e[r] = acc;
            if (JAC) {
#pragma unroll
              for (int c = 0; c < b; c++) {
                T aL = T(0), aR = T(0);
#pragma unroll
                for (int q = r; q < rows; q++) { aL += T(Rw[r * rows + q]) * JL[q * b + c]; aR += T(Rw[r * rows + q]) * JR[q * b + c]; }
                JL[r * b + c] = aL; JR[r * b + c] = aR;
              }
#pragma unroll
              for (int c = 0; c < 3; c++) {
                T am = T(0);
#pragma unroll
                for (int q = r; q < rows; q++) am += T(Rw[r * rows + q]) * Jm[q * 3 + c];
                Jm[r * 3 + c] = am;
              }
            }
          }
        }
      }
      // noiseModel::Robust over the base model above (fp64 handles; compile() refuses the others): one weight per factor from
      // r = |whitened error|_2 (Robust::WhitenSystem, Block reweighting); the cost takes rho(r) in place of r^2 / 2 (Robust::loss).
      // sw = sqrt(w(r)); a null table leaves the arithmetic below as it was
      bool robust = false;
      T sw = T(1);
      if constexpr (IsF64<T>::v) {
        if (a.rob) {
          const int loss = (int)a.rob[2 * (size_t)f];
          double wr = 1.0;
          if (loss != ROBUST_NONE) {
            double r2 = 0.0, rho;
#pragma unroll
            for (int r = 0; r < rows; r++) {
              const double we = e[r] * ((kFullNoise && a.sqi) ? 1.0 : 1.0 / a.sig[(size_t)f * rows + r]);
              r2 += we * we;
            }
            robust_eval(loss, a.rob[2 * (size_t)f + 1], sqrt(r2), wr, rho);
            robust = true;
            sw = sqrt(wr);
            err += 2.0 * rho;      // (halved with the block's sum below)
          }
          if (a.out_w) a.out_w[f] = wr;
        }
      }
#pragma unroll
      for (int r = 0; r < rows; r++) {
        T w = (kFullNoise && a.sqi) ? T(1) : T(1) / T(a.sig[(size_t)f * rows + r]);
        T we = e[r] * w;
        if (robust) { w *= sw; we *= sw; }
        else err += we * we;
        wgt[r] = w;
        if (!JAC && a.rowE32) a.rowE32[row0 + r] = (float)we;
        if (JAC && a.rowLR) {      // (rowLR == null: the inspection call, gpslam_hip_linearize_meas, leaves the row tables alone)
          a.rowE[row0 + r] = we;
          if (a.ld > 0) {
            a.rowLm[row0 + r] = lm;
            for (int q = 0; q < a.ld; q++) a.rowM[(size_t)(row0 + r) * a.ld + q] = w * Jm[r * 3 + q];
          }
        }
      }
    }
    if constexpr (JAC) {
      constexpr int LS = 2 * b + 2;
      __shared__ T stage[2 * 64 * LS];
      __shared__ int srow[128];
      const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
      T *st = stage + wv * 64 * LS, *mine = st + lane * LS;
      srow[threadIdx.x] = row0v;
      if (a.rowLR) {
#pragma unroll
        for (int r = 0; r < rows; r++) {
#pragma unroll
          for (int c = 0; c < b; c++) { mine[c] = wgt[r] * JL[r * b + c]; mine[b + c] = wgt[r] * JR[r * b + c]; }
          wave_store_rows<T, 2 * b>(st, srow + wv * 64, lane, r, a.rowLR);
        }
      }
    }
  }
  const T tot = block_sum(T(0.5) * err);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = tot;
}

// GPInterpolatedGPSFactorPose3 on the structured path, as 16-double lines [Lp | mu | e, p11, p12, l12] (kIRow*) for k_fused_level0<4>,
// which forms the right halves from mu and the interval's GP record -- written for its register count (round 6).  Round 5's form, a
// branch of the general kernel k_meas, kept every row of the factor (rows x 24 doubles), the
// interpolator's three 6 x 6 blocks and the interval's record alive at once: 256 VGPRs + AGPR spill space, ONE wave per SIMD, 0.88 ms
// for 4e6 factors at 0.37 of the HBM roof -- a latency chain nobody covers.  Here the whitening enters through Hp (the rows are
// linear in it: diag(1 / sigma) or the square-root information R of a Gaussian model), so a row is final the moment it is formed;
// the interval's Jinv is dead once xi exists, the record's J and F blocks are requested when the lines are half done, and the pose's
// 12 numbers are the only thing that lives from the first load to the last row.  Same device functions on the same operands as
// interp_pose3 (GaussianProcessInterpolatorPose3.h:57-105, GPInterpolatedGPSFactorPose3.h:66-95): products with the weight
// commute by one rounding.  The interval must carry a GP prior (Plan::lines), body-frame velocities (GpForm::Se3Rec).
// materialise values HERE: an empty volatile asm that "modifies" them keeps the compiler from sinking their computation towards the
// use (and, on a pointer, from hoisting the loads behind it) -- the phases of k_gps_lines below stay phases
template <typename P> __device__ __forceinline__ void pin_ptr(P *&p) { asm volatile("" : "+v"(p)); }
constexpr int kGpsLinesWaves = 2;   // waves per SIMD k_gps_lines is compiled for
// se3_Q (lie.hpp; Pose3utils.cpp:92-113) term by term: the same products and the same order of every sum, each term folded into
// the result before the next one's operands exist (the expression as one statement keeps eight 3 x 3 temporaries alive)
__device__ __forceinline__ M3<double> se3_Q_seq(V3<double> w, V3<double> rho) {
  typedef double T;
  const T th = sqrt(dot(w, w));
  T a, b, c;
  if (fabs(th) > T(1e-5)) {
    const T s = sin(th), co = cos(th);
    const T t2 = th * th, t3 = t2 * th, t4 = t3 * th, t5 = t4 * th;
    a = (th - s) / t3;
    b = (T(1) - T(0.5) * t2 - co) / t4;
    c = T(-0.5) * ((T(1) - T(0.5) * t2 - co) / t4 - T(3) * (th - s - t3 / T(6)) / t5);
  } else {
    a = T(1) / T(6);
    b = T(1) / T(24);
    c = T(-0.5) * (T(1) / T(24) + T(3) / T(120));
  }
  pin(a); pin(b); pin(c);
  const M3<T> X = skew(w), Y = skew(rho);
  M3<T> XY = X * Y, YX = Y * X, XYX = X * YX;
  M3<T> Q = T(-0.5) * Y + a * (XY + YX - XYX);
  pin(Q);
  Q = Q + b * (X * XY + YX * X - T(3) * XYX);
  pin(Q);
  Q = Q + c * (XYX * X + X * XYX);
  return Q;
}
// SENS: some factor of the launch carries a body_P_sensor (a.aidx != null).  Without one Hp = W [0 | R]: its rotational half is
// exactly zero and only the lower block rows of He and Ad(Exp(xi)^-1) are touched -- half of Hp's registers and products.
template <int WAVES, bool SENS>
__global__ void __launch_bounds__(128, WAVES) k_gps_lines(MeasArgs<double> a) {
  typedef double T;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = f < a.count;
  const int ff = live ? f : 0;                   // (idle lanes of the last block recompute factor 0; they store nothing)
  const int i = a.idx[ff];
  const T l12 = a.coef[4 * (size_t)ff + 1], p11 = a.coef[4 * (size_t)ff + 2], p12 = a.coef[4 * (size_t)ff + 3];
  const T *gp = a.gps + (size_t)a.gpidx[i] * kGpsLen;
  const T *gp2 = gp;
  auto m3 = [&](int off) { M3<T> m; for (int q = 0; q < 9; q++) m.m[q] = gp[off + q]; return m; };
  SE3<T> A1;
  V6<T> xi;
  {
    // SoA states through ONE 32-bit byte offset per lane and uniform bases (global_load saddr + voffset): 36 loads with 64-bit
    // per-lane addresses were 72 address registers, more than everything they fetched
    const unsigned off = (unsigned)i * 8u;
    auto ldu = [&](const double *base) { return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + off); };
    T p1[12], p2[12];
#pragma unroll
    for (int k = 0; k < 12; k++) { p1[k] = ldu(a.pose + (size_t)k * a.stride); p2[k] = ldu(a.pose + (size_t)k * a.stride + 1); }
    V6<T> u1, u2;
    {
      T v1[6], v2[6];
#pragma unroll
      for (int k = 0; k < 6; k++) { v1[k] = ldu(a.vel + (size_t)k * a.stride); v2[k] = ldu(a.vel + (size_t)k * a.stride + 1); }
      u1 = as_v6(v1); u2 = as_v6(v2);
    }
    A1 = as_se3(p1);
    const V6<T> r = se3_log(se3_between(A1, as_se3(p2)));
    BL6<T> Jinv;
    Jinv.A = m3(kGpsXA); Jinv.C = m3(kGpsXC); Jinv.D = Jinv.A;
    xi = l12 * u1 + p11 * r + p12 * (Jinv * u2);
  }
  pin(xi);
  SE3<T> ex = se3_exp(xi);
  pin(ex.R); pin(ex.t);
  // the sensor pose and the whitened Hp = W [0 | R_sp] (Ad(S^-1)): three 6-vectors (SENS) or their translational halves
  V6<T> Hp[SENS ? 3 : 1];
  V3<T> hv[SENS ? 1 : 3];
  T ew[3];
  {
    const SE3<T> pose = se3_compose(A1, ex);
    SE3<T> sp = pose;
    BL6<T> AdS;
    bool has_sensor = false;
    if constexpr (SENS) {
      const double *ax = a.aux + (size_t)a.aidx[ff] * kMeasAux;
      has_sensor = ax[17] != 0.0;
      if (has_sensor) {
        T sens[12];
#pragma unroll
        for (int k = 0; k < 12; k++) sens[k] = ax[k];
        const SE3<T> S = as_se3(sens);
        sp = se3_compose(pose, S);
        AdS = se3_adjoint(se3_inverse(S));
      }
    }
    T e[3] = {sp.t.x - a.meas[(size_t)ff * a.mw], sp.t.y - a.meas[(size_t)ff * a.mw + 1], sp.t.z - a.meas[(size_t)ff * a.mw + 2]};
    // W: diag(1 / sigma), or the upper triangular square-root information of a noiseModel::Gaussian (rows <- R rows)
    T W[9] = {T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0)};
    if (a.sqi) {
      const double *Rw = a.sqi + (size_t)ff * 9;
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = r; q < 3; q++) W[r * 3 + q] = Rw[r * 3 + q];
    } else {
#pragma unroll
      for (int r = 0; r < 3; r++) W[r * 4] = T(1) / a.sig[(size_t)ff * 3 + r];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
      T acc = T(0);
      V3<T> hr = {T(0), T(0), T(0)};
#pragma unroll
      for (int q = r; q < 3; q++) {
        acc += W[r * 3 + q] * e[q];
        hr = hr + W[r * 3 + q] * V3<T>{sp.R.m[3 * q], sp.R.m[3 * q + 1], sp.R.m[3 * q + 2]};   // translation(H) = [0, R]
      }
      ew[r] = acc;
      if constexpr (SENS) {
        Hp[r] = {{T(0), T(0), T(0)}, hr};
        if (has_sensor) Hp[r] = rowmul(Hp[r], AdS);
        pin(Hp[r]);
      } else {
        hv[r] = hr;
        pin(hv[r]);
      }
      pin(ew[r]);
    }
  }
  T err = live ? ew[0] * ew[0] + ew[1] * ew[1] + ew[2] * ew[2] : T(0);
  V6<T> mu[3], Lp[3];
  {
    // He = se3_jr(xi) = [[Jr, 0], [Q, Jr]] (rightJacobianPose3, Pose3utils.cpp:182-189), the Q block first
    M3<T> HQ = se3_Q_seq(xi.w, xi.v);
    pin(HQ);
    const M3<T> Jw = so3_jr(xi.w);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      if constexpr (SENS) mu[r] = rowmul(Hp[r], BL6<T>{Jw, HQ, Jw});
      else mu[r] = {rowmul(hv[r], HQ), rowmul(hv[r], Jw)};
      pin(mu[r]);
    }
  }
  {
    const BL6<T> Hc21 = se3_adjoint(se3_inverse(ex));
#pragma unroll
    for (int r = 0; r < 3; r++) {
      if constexpr (SENS) Lp[r] = rowmul(Hp[r], Hc21);
      else Lp[r] = {rowmul(hv[r], Hc21.C), rowmul(hv[r], Hc21.D)};
      pin(Lp[r]);
    }
  }
  pin_ptr(gp2);      // the record's J and F blocks are requested from here on, not before
  {   // Lp += mu (p11 J + p12 F J) as (p11 mu + p12 (mu F)) J, one 3 x 3 block of the record at a time: F J is never formed and no
      // two blocks are alive together (mu F = [mu_w FA + mu_v FC | mu_v FD], b J = [b_w JA + b_v JC | b_v JA])
    auto n3 = [&](int off) { M3<T> m; for (int q = 0; q < 9; q++) m.m[q] = gp2[off + q]; return m; };
    V6<T> bq[3];
    {
      M3<T> blk = n3(kGpsFA);
#pragma unroll
      for (int r = 0; r < 3; r++) { bq[r].w = rowmul(mu[r].w, blk); pin(bq[r].w); }
      blk = n3(kGpsFC);
#pragma unroll
      for (int r = 0; r < 3; r++) { bq[r].w = p11 * mu[r].w + p12 * (bq[r].w + rowmul(mu[r].v, blk)); pin(bq[r].w); }
      blk = n3(kGpsFD);
#pragma unroll
      for (int r = 0; r < 3; r++) { bq[r].v = p11 * mu[r].v + p12 * rowmul(mu[r].v, blk); pin(bq[r].v); }
    }
    pin_ptr(gp2);
    {
      M3<T> blk = n3(kGpsJA);
#pragma unroll
      for (int r = 0; r < 3; r++) { Lp[r].w = Lp[r].w + rowmul(bq[r].w, blk); Lp[r].v = Lp[r].v + rowmul(bq[r].v, blk); pin(Lp[r]); }
      blk = n3(kGpsJC);
#pragma unroll
      for (int r = 0; r < 3; r++) { Lp[r].w = Lp[r].w + rowmul(bq[r].v, blk); pin(Lp[r].w); }
    }
  }
  __shared__ T istage[2 * 64 * 20];
  __shared__ int isrow[128];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  T *st = istage + wv * 64 * 20, *mine = st + lane * 20;
  isrow[threadIdx.x] = live ? a.row0[f] : -1;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    put_v6(Lp[r], mine + kIRowLp); put_v6(mu[r], mine + kIRowMu);
    mine[kIRowE] = ew[r]; mine[kIRowP11] = p11; mine[kIRowP12] = p12; mine[kIRowL12] = l12;
    wave_store_part<T, kIRowLen, 16, 20, true>(st, isrow + wv * 64, lane, r, 0, a.rowI);
  }
  const T tot = block_sum(T(0.5) * err);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = tot;
}

// ------------------------------------------------------------------ landmark border (Schur complement)

// TR: type of the Jacobian row tables (float on fp32 handles, whose normal equations and solver stay fp64)
template <typename T, typename TR = T> struct LmArgs {
  int N, R, B, L, ld, nl;   // R = 1 + nl
  int Nx;                   // solution slots in x: N, or N + 1 when a halo state follows the segment
  const TR *rowLR, *rowE, *rowM;
  const int *lmrow;         // row ids of rows that touch a landmark, grouped by landmark
  const int *lmrow_state;   // left state of each such row
  const int *lmrow_ptr;     // L + 1
  int nlmrows;
  const int *chunk_lm, *chunk_j0, *chunk_j1;   // row chunks of the landmark rows (each inside one landmark)
  const int *chunk_ptr;     // L + 1: chunks of landmark l are chunk_ptr[l] .. chunk_ptr[l + 1]
  int nchunks;
  T *part;                  // nchunks x ld x R partial sums of the Schur complement
  T *x;                     // level-0 solutions, N x R x B (column 0 is corrected in place)
  T *t;                     // nlmrows x R
  // landmark priors
  int npri;
  const int *pri_lm;
  const double *pri_meas, *pri_sig;
  double *lmk;              // L x ld (fp64 like the states)
  T *S;                     // nl x (nl + 1): column 0 = rhs, columns 1.. = Schur complement
  T *gL;                    // nl (undamped gradient, for LM)
  T *dL;                    // nl solution
  T lambda;
  int *flag;
  T *partial;
};

// t[j][c] = JL_rho . X_s[:, c] + JR_rho . X_{s+1}[:, c]
template <typename T, typename TR = T> __global__ void __launch_bounds__(128) k_lm_t(LmArgs<T, TR> a) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = tid / a.R, c = tid - j * a.R;
  if (j >= a.nlmrows) return;
  const int rho = a.lmrow[j], s = a.lmrow_state[j];
  const TR *row = a.rowLR + (size_t)rho * 2 * a.B;
  const T *x0 = a.x + ((size_t)s * a.R + c) * a.B;
  T acc = T(0);
  for (int k = 0; k < a.B; k++) acc += row[k] * x0[k];
  if (s + 1 < a.Nx) {
    const T *x1 = a.x + ((size_t)(s + 1) * a.R + c) * a.B;
    for (int k = 0; k < a.B; k++) acc += row[a.B + k] * x1[k];
  }
  a.t[(size_t)j * a.R + c] = acc;
}

// Landmark Schur complement S[al][c]: c = 0 -> rhs gL - B^T x0; c >= 1 -> (H_LL + lambda I - B^T Z)[al][c-1], in two
// stages with a fixed summation order: a landmark may be seen from tens of thousands of rows (Plaza-rate ranges on a
// 1e6-state chain: 55k rows per landmark), so the rows are cut into chunks that one workgroup each reduces, thread
// (q, c) = (component of the landmark, column) running down the chunk; a second kernel adds the chunks of a landmark
// in order, the priors and the damping.
constexpr int kLmChunk = 64;
template <typename T, typename TR = T> __global__ void __launch_bounds__(256) k_lm_reduce_part(LmArgs<T, TR> a) {
  const int ch = blockIdx.x;
  const int W = a.ld * a.R;                       // (q, c) pairs, <= 84
  const int nsub = 256 / W;                       // row phases per pair (the loop is a chain of dependent loads)
  const int sub = threadIdx.x / W, qc = threadIdx.x - sub * W;
  const int q = qc / a.R, c = qc - q * a.R;
  __shared__ T red[2][256];
  T acc = T(0), g = T(0);
  if (sub < nsub) {
    const int lm = a.chunk_lm[ch];
    const int cl = c - 1;
    const bool same = (c >= 1) && (cl / a.ld == lm);
    const int q2 = same ? cl - lm * a.ld : 0;
    for (int j = a.chunk_j0[ch] + sub; j < a.chunk_j1[ch]; j += nsub) {
      const int rho = a.lmrow[j];
      const T m = a.rowM[(size_t)rho * a.ld + q];
      if (c == 0) g -= m * a.rowE[rho];
      else if (same) acc += m * a.rowM[(size_t)rho * a.ld + q2];
      acc -= m * a.t[(size_t)j * a.R + c];
    }
    red[0][threadIdx.x] = acc;
    red[1][threadIdx.x] = g;
  }
  __syncthreads();
  if (sub == 0) {                                  // fixed order over the phases
    T sa = T(0), sg = T(0);
    for (int u = 0; u < nsub; u++) { sa += red[0][u * W + qc]; sg += red[1][u * W + qc]; }
    a.part[((size_t)ch * a.ld + q) * a.R + c] = sa + sg;          // c = 0: gL - B^T x0
    if (c == 0) a.part[((size_t)a.nchunks * a.ld + (size_t)ch * a.ld + q) * a.R] = sg;   // gL alone feeds the LM model
  }
}
// one wave per (al, c): lanes stride over the chunks of the landmark, then a fixed-order wave sum
template <typename T, typename TR = T> __global__ void __launch_bounds__(64) k_lm_reduce(LmArgs<T, TR> a) {
  const int al = blockIdx.x / a.R, c = blockIdx.x - al * a.R;
  const int lm = al / a.ld, q = al - lm * a.ld;
  const int cl = c - 1;
  T acc = T(0), g = T(0);
  for (int ch = a.chunk_ptr[lm] + (int)threadIdx.x; ch < a.chunk_ptr[lm + 1]; ch += 64) {
    acc += a.part[((size_t)ch * a.ld + q) * a.R + c];
    if (c == 0) g += a.part[((size_t)a.nchunks * a.ld + (size_t)ch * a.ld + q) * a.R];
  }
  acc = wave_sum(acc);
  g = wave_sum(g);
  if (threadIdx.x != 0) return;
  for (int k = 0; k < a.npri; k++) {
    if (a.pri_lm[k] != lm) continue;
    const T w = T(1) / a.pri_sig[(size_t)k * a.ld + q];
    if (c == 0) { const T gp = -w * w * (a.lmk[(size_t)lm * a.ld + q] - a.pri_meas[(size_t)k * a.ld + q]); g += gp; acc += gp; }
    else if (cl == al) acc += w * w;
  }
  if (c == 0) a.gL[al] = g;
  else if (cl == al) acc += a.lambda;
  a.S[(size_t)al * a.R + c] = acc;
}

// Dense SPD solve of the (small) landmark system, S = columns 1..nl of a.S (upper part), rhs = column 0 -> dL.
// One wave, right-looking Cholesky in LDS: step j scales column j (lane per row) and applies the rank-1 update to the
// trailing block and to the rhs (lane per entry); then the back-substitution.  nl <= 27.
template <typename T, typename TR = T> __global__ void __launch_bounds__(64) k_lm_solve(LmArgs<T, TR> a) {
  constexpr int NM = kMaxRhs - 1;
  __shared__ T M[NM][NM + 1];      // lower triangle becomes L; +1: no bank conflicts down a column
  __shared__ T y[NM];
  const int n = a.nl, R = a.R, lane = threadIdx.x;
  for (int idx = lane; idx < n * n; idx += 64) {
    const int i = idx / n, j = idx - i * n;
    M[i][j] = (j <= i) ? a.S[(size_t)j * R + 1 + i] : T(0);         // S is stored by its upper part: S[j][i], j <= i
  }
  for (int i = lane; i < n; i += 64) y[i] = a.S[(size_t)i * R];
  wave_lds_sync();
  for (int j = 0; j < n; j++) {
    T dd = M[j][j];
    if (!(dd > T(0))) { if (lane == 0) *a.flag = 1; dd = T(1); }
    const T l = sqrt(dd), linv = T(1) / l;
    wave_lds_sync();
    for (int i = j + lane; i < n; i += 64) M[i][j] = (i == j) ? l : M[i][j] * linv;
    if (lane == 0) y[j] *= linv;
    wave_lds_sync();
    const int m = n - j - 1;                                        // trailing block (j+1 .. n-1)^2, lower part, + rhs
    for (int idx = lane; idx < m * m + m; idx += 64) {
      if (idx < m * m) {
        const int i = j + 1 + idx / m, k = j + 1 + idx % m;
        if (k <= i) M[i][k] -= M[i][j] * M[k][j];
      } else {
        const int i = j + 1 + (idx - m * m);
        y[i] -= M[i][j] * y[j];
      }
    }
    wave_lds_sync();
  }
  // L^T dL = y
  for (int i = n - 1; i >= 0; i--) {
    if (lane == 0) {
      const T v = y[i] / M[i][i];
      y[i] = v;
      a.dL[i] = v;
    }
    wave_lds_sync();
    const T v = y[i];
    for (int k = lane; k < i; k += 64) y[k] -= M[i][k] * v;
    wave_lds_sync();
  }
}

// delta_p = x0 - Z dL  (in place in column 0 of x)
template <typename T, typename TR = T> __global__ void __launch_bounds__(256) k_lm_correct(LmArgs<T, TR> a) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = tid / a.B, k = tid - s * a.B;
  if (s >= a.N) return;
  T *xs = a.x + (size_t)s * a.R * a.B;
  T v = xs[k];
  for (int q = 0; q < a.nl; q++) v -= xs[(size_t)(1 + q) * a.B + k] * a.dL[q];
  xs[k] = v;
}

// landmarks += dL; out[0] = max |dL| (single block)
template <typename T, typename TR = T> __global__ void __launch_bounds__(64) k_lm_update(LmArgs<T, TR> a, double *out_max) {
  T mx = T(0);
  const bool bad = a.flag && *a.flag;          // indeterminate system: leave the landmarks where they are
  for (int i = threadIdx.x; i < a.nl; i += 64) {
    if (!bad) a.lmk[i] += a.dL[i];
    mx = fmax(mx, abs_or_inf(a.dL[i]));
  }
  mx = wave_max(mx);
  if (threadIdx.x == 0) *out_max = fmax(*out_max, (double)mx);
}

// error of the landmark priors (PriorFactor<Point>), single block
template <typename T, typename TR = T> __global__ void __launch_bounds__(128) k_lmprior_err(LmArgs<T, TR> a) {
  T err = T(0);
  for (int k = threadIdx.x; k < a.npri; k += 128)
    for (int q = 0; q < a.ld; q++) {
      const T we = (a.lmk[(size_t)a.pri_lm[k] * a.ld + q] - a.pri_meas[(size_t)k * a.ld + q]) / a.pri_sig[(size_t)k * a.ld + q];
      err += we * we;
    }
  const T tot = block_sum(T(0.5) * err);
  if (threadIdx.x == 0) a.partial[0] = tot;
}

// ---- small utilities for Levenberg-Marquardt
// partial[b] = sum over this block of a[i] * b[i]  (stride-aware: element i lives at a[i * sa], b[i * sb])
// the three dot products of a Levenberg-Marquardt trial in one launch (round 3): x . y0, x . y1 (y1 may be null), x . x, each with
// k_dot's partition into per-block partial sums -- partial[b], partial[nb + b], partial[2 nb + b] -- so that k_final_reduce3 adds
// them up in k_final_reduce's order: the model-fidelity test sees bit-identical numbers
template <typename T> __global__ void __launch_bounds__(256) k_dot3(const T *x, const T *y0, const T *y1, int n, T *partial) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nb = gridDim.x;
  const T xi = (i < n) ? x[i] : T(0);
  const T t0 = block_sum((i < n) ? xi * y0[i] : T(0));
  __syncthreads();
  const T t1 = block_sum((i < n && y1 != nullptr) ? xi * y1[i] : T(0));
  __syncthreads();
  const T t2 = block_sum((i < n) ? xi * xi : T(0));
  if (threadIdx.x == 0) { partial[blockIdx.x] = t0; partial[nb + blockIdx.x] = t1; partial[2 * nb + blockIdx.x] = t2; }
}
// block b: out[slot[b]] = sum of in[b * n .. b * n + n) in k_final_reduce's order
template <typename T> __global__ void __launch_bounds__(256) k_final_reduce3(const T *in, int n, double *out, int s0, int s1, int s2) {
  const T *p = in + (size_t)blockIdx.x * n;
  const T acc = strided_fold(p, n, 0);
  const T r = block_sum(acc);
  const int slot = blockIdx.x == 0 ? s0 : (blockIdx.x == 1 ? s1 : s2);
  if (threadIdx.x == 0 && slot >= 0) out[slot] = (double)r;
}
template <typename T> __global__ void __launch_bounds__(256) k_dot(const T *x, const T *y, int n, T *partial) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const T v = (i < n) ? x[i] * y[i] : T(0);
  const T tot = block_sum(v);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}
// gather column 0 of the N x R x B solution array into a dense N x B vector
template <typename T> __global__ void __launch_bounds__(256) k_gather_delta(const T *x, int N, int R, int B, T *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * B) return;
  const int s = i / B, k = i - s * B;
  out[i] = x[(size_t)s * R * B + k];
}

// ------------------------------------------------------------------ K3: assemble normal equations

template <typename T, typename TR = T> struct AsmArgs {
  int N, R;               // states, rhs columns (1 + border)
  const int *rowptr;      // N + 2 entries; rows of left state s: [rowptr[s], rowptr[s+1]); rowptr[-1] handled by s > 0
  const TR *rowLR, *rowE;
  const int *crowptr;     // compact rows (velocity-free Jacobians) of left state s: [crowptr[s], crowptr[s+1])
  const TR *rowC, *rowCE; // Mc x B = [d/dpose_left (B/2) | d/dpose_right (B/2)], Mc
  const TR *rowM;         // M x ld (border) or null
  const int *rowLm;       // landmark id per row or -1
  int ld;
  T *blk;                 // N records [D | O | G]
  T *gsave;               // N x B copy of the gradient column (for the LM model-fidelity test) or null
  T *halo_add;            // segment sharding: [RD | Rg] the rows of state N-1 owe to the next rank's first state
  // block size 6, fp64: the GP priors as structured records (kGp3*; K1 wrote no rows for them) or null
  const T *gps3;          // gp_count + 1 records, the last one all zeros
  const int *gpidx;       // record of the GP prior whose left state is s, or -1 (N + 2 entries)
  int gp_count;
  const T *Ud;            // chol_upper(Qc^-1), row-major 3 x 3
};

// Wave-cooperative assembly, every row fetched once.  A wave owns G - 1 = 64 / B - 1 consecutive states plus, in
// its first lane group, the state before them as a "ghost" that only contributes its rows' right halves.  The B
// lanes of a group each load ONE element of the left and of the right half of their state's current Jacobian row
// (coalesced 8-byte-per-lane loads, two rows in flight) and publish them in a per-wave LDS exchange buffer; a lane
// then reads back its own row's left half (-> D_s += L^T L, O_s += R^T L) and the right half published by the
// group of state s - 1 (-> D_s += R^T R).  Compared with letting every group re-read the rows of s - 1 this
// removes the second pass over the row table (2x HBM over-fetch measured, profiles/round1_v3) and a third of the
// loop iterations.  DS operations of one wave execute in order, so no barrier is needed; two buffers alternate.
template <typename T, int B, int WPB = 4, typename TR = T>
__global__ void __launch_bounds__(64 * WPB) k_assemble_ghost(AsmArgs<T, TR> a) {
  constexpr int G = 64 / B;                       // lane groups per wave (the first one is the ghost)
  static_assert(G >= 2, "needs at least one real state per wave");
  const int lane = threadIdx.x & 63;
  // blocks walk the chain from its END: the rows written last by the linearisation are the ones still in the
  // memory-side cache
  const int wave = (int)(((gridDim.x - 1 - blockIdx.x) * blockDim.x + threadIdx.x) >> 6);
  const int g = lane / B, c = lane - g * B;
  const int nstates = a.N + (a.halo_add ? 1 : 0);
  const int s = wave * (G - 1) + g - 1;           // ghost: the state before the wave's first
  const bool owner = (g < G) && s >= 0 && s < a.N;           // has rows to load
  const bool out = (g >= 1) && (g < G) && s < nstates;       // produces a block (or the halo addend)
  const int sc = out ? s : 0;
  const int gb = g * B, gp = (g >= 1 ? g - 1 : 0) * B;
  int rp_s = 0, n_own = 0;
  if (owner) {
    rp_s = a.rowptr[s];
    n_own = a.rowptr[s + 1] - rp_s;
  }
  // structured GP prior of the state (block size 6): its six rows are formed from the record below, the row loop starts behind them
  int gq = -1;
  if constexpr (B == 6 && std::is_same<T, double>::value && std::is_same<TR, double>::value) {
    if (a.gps3 && owner) gq = a.gpidx[s];
    if (gq >= 0) { rp_s += B; n_own -= B; }
  }
  int n_max = n_own;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_max = max(n_max, __shfl_xor(n_max, o, 64));
  n_max = __builtin_amdgcn_readfirstlane(n_max);
  const int rp_prev = __shfl(rp_s, gp, 64);       // first row of state s - 1 (landmark columns of its rows)
  const int n_prev = __shfl(n_own, gp, 64);
  T D[B], O[B];
  T gsum = T(0);
#pragma unroll
  for (int k = 0; k < B; k++) { D[k] = T(0); O[k] = T(0); }
  constexpr int XS = 128 + ((G + 1) & ~1);        // per wave and parity: L[64] | R[64] | e[G]
  __shared__ T xch[WPB][2][XS];
  T *xw = &xch[threadIdx.x >> 6][0][0];
  const int BS = 2 * B * B + B * a.R;
  T *bp = a.blk + (size_t)sc * BS;
  const bool isblk = out && sc < a.N;
  // rhs columns: of this state's record, or -- for the virtual state behind the segment -- of the addend owed to the
  // next rank's first state (the rows of the last interval carry landmark columns too)
  T *gcol = isblk ? bp + 2 * B * B : ((out && a.halo_add) ? a.halo_add + B * B : nullptr);
  if (gcol) for (int r = 1; r < a.R; r++) gcol[r * B + c] = T(0);
  // loads are unconditional (row index clamped to the state's last row, the ghost group re-reads its R element
  // instead of an L element); validity is applied when the values are consumed.  A predicated load would make the
  // loaded value a phi with zero, and the copy that implements the phi waits for the load.
  const int n_last = max(n_own - 1, 0);
  auto ld = [&](int i, T &Lc, T &Rc, T &e) {
    const int rho = rp_s + min(i, n_last);
    const TR *row = a.rowLR + (size_t)rho * 2 * B;
    Lc = row[g >= 1 ? c : B + c];
    Rc = row[B + c];
    e = a.rowE[rho];
  };
  auto step = [&](int i, const bool valid, const T Lraw, const T Rraw, const T eraw) {
    const T Lc = (valid && g >= 1) ? Lraw : T(0), Rc = valid ? Rraw : T(0), e = valid ? eraw : T(0);
    T *buf = xw + (i & 1) * XS;
    buf[lane] = Lc;
    buf[64 + lane] = Rc;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const T *Lrow = buf + gb;
    const T *Prow = buf + 64 + gp;                // right half of the current row of state s - 1
    const T Pc = Prow[c];
    const T ep = __shfl(e, gp, 64);               // e of state s - 1's current row (no branch: keeps the step one block)
#pragma unroll
    for (int k = 0; k < B; k++) {
      if (B > 8 && k == B / 2) __builtin_amdgcn_sched_barrier(0);   // halves the LDS read-back registers live at once
      const T Lk = Lrow[k];
      D[k] += Lc * Lk;
      O[k] += Rc * Lk;
      D[k] += Pc * Prow[k];
    }
    gsum -= Lc * e;
    gsum -= Pc * ep;
  };
  if constexpr (B == 6 && std::is_same<T, double>::value && std::is_same<TR, double>::value) {
    if (a.gps3) {
      // Lane c of the state's group holds column c of the six rows [A1 | kLt U | A3 | kRt U; 0 | kLb U | 0 | kRb U]: a pose lane
      // (c < 3) its column of A1 / A3 (and nothing in the bottom rows), a velocity lane column c - 3 of U times the record's
      // four coefficients.  States without a GP prior (and idle groups) read the all-zero record.
      const bool pc = c < 3;
      const int c3 = pc ? c : c - 3;
      const T *rec = a.gps3 + (size_t)(gq >= 0 ? gq : a.gp_count) * kGp3Len;
      T colL[3], colR[3], ew[6];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const T uk = a.Ud[3 * k + c3];
        colL[k] = pc ? rec[kGp3A1 + 3 * k + c3] : uk;
        colR[k] = pc ? rec[kGp3A3 + 3 * k + c3] : uk;
      }
      const T mLt = pc ? T(1) : rec[kGp3S + 0], mRt = pc ? T(1) : rec[kGp3S + 1];
      const T mLb = pc ? T(0) : rec[kGp3S + 2], mRb = pc ? T(0) : rec[kGp3S + 3];
#pragma unroll
      for (int i = 0; i < 6; i++) ew[i] = rec[kGp3E + i];
#pragma unroll
      for (int i = 0; i < 6; i++) {
        step(i, true, (i < 3 ? mLt : mLb) * colL[i % 3], (i < 3 ? mRt : mRb) * colR[i % 3], ew[i]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // PF register sets rotate by full unrolling (no register copies: a copy of a set whose load is still in flight
  // would wait for it and cut the prefetch distance to one iteration -- measured 1000-2400 cycles of exposed
  // latency per row before this change)
  constexpr int PF = 3;
  T rL[PF], rR[PF], rE[PF];
  if (n_max > 0) {                                // (an empty row table may be a null pointer)
#pragma unroll
    for (int j = 0; j < PF; j++) {
      ld(j, rL[j], rR[j], rE[j]);
      __builtin_amdgcn_sched_barrier(0);          // issue order = consumption order (vmcnt counts in order)
    }
  }
  for (int i0 = 0; i0 < n_max; i0 += PF) {
#pragma unroll
    for (int j = 0; j < PF; j++) {
      step(i0 + j, i0 + j < n_own, rL[j], rR[j], rE[j]);          // steps past n_max exchange zeros
      ld(i0 + j + PF, rL[j], rR[j], rE[j]);
      __builtin_amdgcn_sched_barrier(0);          // keeps the next step's LDS reads from being hoisted (VGPRs)
    }
  }
  // compact rows: the same exchange with half-width rows; only the pose rows / columns of D_s and O_s are touched
  {
    constexpr int Dh = B / 2;
    int crp = 0, cn = 0;
    if (owner) {
      crp = a.crowptr[s];
      cn = a.crowptr[s + 1] - crp;
    }
    int cmax = cn;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cmax = max(cmax, __shfl_xor(cmax, o, 64));
    cmax = __builtin_amdgcn_readfirstlane(cmax);
    const int cn_last = max(cn - 1, 0);
    const int cc = c < Dh ? c : 0;
    auto ldc = [&](int i, T &Lc, T &Rc, T &e) {
      const int rho = crp + min(i, cn_last);
      const TR *row = a.rowC + (size_t)rho * B;
      Lc = row[g >= 1 ? cc : Dh + cc];
      Rc = row[Dh + cc];
      e = a.rowCE[rho];
    };
    T cL[PF], cR[PF], cE[PF];
    if (cmax > 0) {
#pragma unroll
      for (int j = 0; j < PF; j++) {
        ldc(j, cL[j], cR[j], cE[j]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    auto cstep = [&](int i, const T Lraw, const T Rraw, const T eraw) {
      const bool valid = i < cn;
      const T Lc = (valid && g >= 1 && c < Dh) ? Lraw : T(0), Rc = (valid && c < Dh) ? Rraw : T(0), e = valid ? eraw : T(0);
      T *buf = xw + (i & 1) * XS;
      buf[lane] = Lc;
      buf[64 + lane] = Rc;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const T *Lrow = buf + gb;
      const T *Prow = buf + 64 + gp;
      const T Pc = Prow[c];
      const T ep = __shfl(e, gp, 64);               // e of state s - 1's current row (no branch: keeps the step one block)
#pragma unroll
      for (int k = 0; k < Dh; k++) {
        const T Lk = Lrow[k];
        D[k] += Lc * Lk;
        O[k] += Rc * Lk;
        D[k] += Pc * Prow[k];
      }
      gsum -= Lc * e;
      gsum -= Pc * ep;
    };
    for (int i0 = 0; i0 < cmax; i0 += PF) {
#pragma unroll
      for (int j = 0; j < PF; j++) {
        cstep(i0 + j, cL[j], cR[j], cE[j]);
        ldc(i0 + j + PF, cL[j], cR[j], cE[j]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // landmark columns of the rows that have one (range / projection factors; a small minority of the rows): a second
  // pass that re-reads just those rows, own rows first, then the rows of state s - 1 -- kept out of the exchange
  // loop so that its steps stay branch-free
  if (a.rowM && gcol) {
    for (int i = 0; i < n_own; i++) {
      const int rho = rp_s + i;
      const int lm = a.rowLm[rho];
      if (lm < 0) continue;
      const T Lc = a.rowLR[(size_t)rho * 2 * B + c];
      for (int q = 0; q < a.ld; q++) gcol[(1 + lm * a.ld + q) * B + c] += Lc * a.rowM[(size_t)rho * a.ld + q];
    }
    for (int i = 0; i < n_prev; i++) {
      const int rho = rp_prev + i;
      const int lm = a.rowLm[rho];
      if (lm < 0) continue;
      const T Pc = a.rowLR[(size_t)rho * 2 * B + B + c];
      for (int q = 0; q < a.ld; q++) gcol[(1 + lm * a.ld + q) * B + c] += Pc * a.rowM[(size_t)rho * a.ld + q];
    }
  }
  if (out && sc == a.N) {   // halo: what the rows of state N-1 owe the neighbour's first state
#pragma unroll
    for (int k = 0; k < B; k++) a.halo_add[c * B + k] = D[k];
    a.halo_add[B * B + c] = gsum;
  }
  // [D | O | g] leave through a per-wave LDS image of the G - 1 records, then as 16-byte-per-lane stores that are
  // contiguous within a record.  Writing a lane's row of D directly (16-byte pieces at a B * 8 byte stride, one write
  // request per lane) cost 0.085 of the kernel's 0.20 ms on the benchmark chain.
  constexpr int RS = 2 * B * B + B;
  __shared__ T stg[WPB][(G - 1) * RS];
  T *sw = &stg[threadIdx.x >> 6][0];
  if (isblk) {
    T *r = sw + (g - 1) * RS;
#pragma unroll
    for (int k = 0; k < B; k++) { r[c * B + k] = D[k]; r[B * B + c * B + k] = O[k]; }
    r[2 * B * B + c] = gsum;
    if (a.gsave) a.gsave[(size_t)sc * B + c] = gsum;
  }
  wave_lds_sync();
  typedef T V2 __attribute__((ext_vector_type(2)));
  const int s_first = wave * (G - 1);
  constexpr int NPAIR = (G - 1) * RS / 2;
  static_assert(RS % 2 == 0, "records are copied in pairs");
#pragma unroll
  for (int t = 0; t < (NPAIR + 63) / 64; t++) {
    const int q = t * 64 + lane;
    const int j = (2 * q) / RS, off = 2 * q - j * RS;
    if (q < NPAIR && s_first + j < a.N)
      // non-temporal: the records are next touched by another kernel, and kept out of the caches they leave the rows
      // this kernel still has to read where the linearisation left them (0.150 -> 0.133 ms; the elimination pays 10 us)
      __builtin_nontemporal_store(*reinterpret_cast<const V2 *>(sw + 2 * q), reinterpret_cast<V2 *>(a.blk + (size_t)(s_first + j) * BS + off));
  }
}

// ------------------------------------------------------------------ trajectory queries

template <typename T> struct QueryArgs {
  const double *pose, *vel;   // SoA states
  int stride, count;
  const int *left;       // query q lies in the interval (left[q], left[q] + 1)
  const double *coef;        // count x 4: l11, l12, p11, p12 for (dt[q], tau[q])
  int vw;                // Pose3 only: velocities are world-frame [v; w]
  T *out;                // count x pose_dim (AoS, the layout of gpslam_hip_get_states' rows)
  T *out_H;              // JAC: count x 4 x d x d = H1..H4 of interpolatePose (GaussianProcessInterpolatorPose3.h:82-98)
};

// Batched GaussianProcessInterpolator{Linear,Pose2,Pose3,Rot3}::interpolatePose without Jacobians (the public
// query use of the interpolators, gpslam.h:57-86): thread per query.
template <typename T, int MF, bool JAC = false>
__global__ void __launch_bounds__(128) k_interp_query(QueryArgs<T> a) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.count) return;
  const int i = a.left[q];
  const ICoef<T> k = {T(a.coef[4 * (size_t)q]), T(a.coef[4 * (size_t)q + 1]), T(a.coef[4 * (size_t)q + 2]), T(a.coef[4 * (size_t)q + 3])};
  T p1[pd], p2[pd], v1[d], v2[d];
#pragma unroll
  for (int c = 0; c < pd; c++) { p1[c] = a.pose[(size_t)c * a.stride + i]; p2[c] = a.pose[(size_t)c * a.stride + i + 1]; }
#pragma unroll
  for (int c = 0; c < d; c++) { v1[c] = a.vel[(size_t)c * a.stride + i]; v2[c] = a.vel[(size_t)c * a.stride + i + 1]; }
  if constexpr (MF == POSE3) {
    if (a.vw) {
      T b1[6], b2[6];
      vw_to_vb(p1, v1, b1);
      vw_to_vb(p2, v2, b2);
#pragma unroll
      for (int c = 0; c < 6; c++) { v1[c] = b1[c]; v2[c] = b2[c]; }
    }
  }
  T *o = a.out + (size_t)q * pd;
  T *oh = JAC ? a.out_H + (size_t)q * 4 * d * d : nullptr;
  if constexpr (MF == LINEAR2 || MF == LINEAR3) {
    // p(tau) = Lambda_1 [p1; v1] + Psi_1 [p2; v2]   (GaussianProcessInterpolatorLinear.h:70-90)
#pragma unroll
    for (int c = 0; c < d; c++) o[c] = k.l11 * p1[c] + k.l12 * v1[c] + k.p11 * p2[c] + k.p12 * v2[c];
    if (JAC) {     // H_k = the d x d blocks of Lambda_1, Psi_1 (:83-86): scalar multiples of I for the shared Qc
      const T cf[4] = {k.l11, k.l12, k.p11, k.p12};
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int r = 0; r < d; r++)
#pragma unroll
          for (int c = 0; c < d; c++) oh[(m * d + r) * d + c] = (r == c) ? cf[m] : T(0);
    }
  } else if constexpr (MF == POSE2) {
    Interp3Out<T, JAC> jo;
    const SE2<T> r = interp_pose2<T, JAC>(p1, v1, p2, v2, k, jo);
    o[0] = r.x; o[1] = r.y; o[2] = r.th;
    if (JAC) { put_m3(jo.H1, oh, 3, 0, 0); put_m3(jo.H2, oh + 9, 3, 0, 0); put_m3(jo.H3, oh + 18, 3, 0, 0); put_m3(jo.H4, oh + 27, 3, 0, 0); }
  } else if constexpr (MF == ROT3) {
    Interp3Out<T, JAC> jo;
    const M3<T> r = interp_rot3<T, JAC>(p1, v1, p2, v2, k, jo);
#pragma unroll
    for (int c = 0; c < 9; c++) o[c] = r.m[c];
    if (JAC) { put_m3(jo.H1, oh, 3, 0, 0); put_m3(jo.H2, oh + 9, 3, 0, 0); put_m3(jo.H3, oh + 18, 3, 0, 0); put_m3(jo.H4, oh + 27, 3, 0, 0); }
  } else if constexpr (MF == ROT3_BIAS) {
    // the rotation is interpolated (GaussianProcessInterpolatorRot3); the bias slot returns the left state's bias, the one
    // an AHRSFactor over this interval uses
    Interp3Out<T, JAC> jo;
    const M3<T> r = interp_rot3<T, JAC>(p1, v1, p2, v2, k, jo);
#pragma unroll
    for (int c = 0; c < 9; c++) o[c] = r.m[c];
#pragma unroll
    for (int c = 0; c < 3; c++) o[9 + c] = p1[9 + c];
    if (JAC) {
#pragma unroll
      for (int c = 0; c < 4 * 36; c++) oh[c] = T(0);
      put_m3(jo.H1, oh, 6, 0, 0); put_m3(jo.H2, oh + 36, 6, 0, 0); put_m3(jo.H3, oh + 72, 6, 0, 0); put_m3(jo.H4, oh + 108, 6, 0, 0);
#pragma unroll
      for (int c = 0; c < 3; c++) oh[(3 + c) * 6 + 3 + c] = T(1);
    }
  } else {
    Interp6Out<T, JAC> jo;
    const SE3<T> r = interp_pose3<T, JAC>(p1, v1, p2, v2, k, jo);
#pragma unroll
    for (int c = 0; c < 9; c++) o[c] = r.R.m[c];
    o[9] = r.t.x; o[10] = r.t.y; o[11] = r.t.z;
    if (JAC) {
#pragma unroll
      for (int c = 0; c < 4 * 36; c++) oh[c] = T(0);
      put_bl6(jo.H1, oh, 6, 0, 0); put_bl6(jo.H2, oh + 36, 6, 0, 0); put_bl6(jo.H3, oh + 72, 6, 0, 0); put_bl6(jo.H4, oh + 108, 6, 0, 0);
      if (a.vw) {   // chain rule through convertVWtoVb, one 12-wide [d/dpose | d/dVb] segment per output row and state
#pragma unroll
        for (int rr = 0; rr < 6; rr++) {
          T seg[12];
#pragma unroll
          for (int c = 0; c < 6; c++) { seg[c] = oh[rr * 6 + c]; seg[6 + c] = oh[36 + rr * 6 + c]; }
          vw_row_transform(p1, v1, seg);
#pragma unroll
          for (int c = 0; c < 6; c++) { oh[rr * 6 + c] = seg[c]; oh[36 + rr * 6 + c] = seg[6 + c]; }
#pragma unroll
          for (int c = 0; c < 6; c++) { seg[c] = oh[72 + rr * 6 + c]; seg[6 + c] = oh[108 + rr * 6 + c]; }
          vw_row_transform(p2, v2, seg);
#pragma unroll
          for (int c = 0; c < 6; c++) { oh[72 + rr * 6 + c] = seg[c]; oh[108 + rr * 6 + c] = seg[6 + c]; }
        }
      }
    }
  }
}

// Batched GaussianProcessInterpolatorLinear<D>::interpolateVelocity (GaussianProcessInterpolatorLinear.h:106-126): the bottom
// block rows of Lambda and Psi.  coef = (l21, l22, p21, p22) per query; H_k = those scalars times I (:117-120).
template <typename T, int MF>
__global__ void __launch_bounds__(128) k_interp_velocity(QueryArgs<T> a) {
  constexpr int d = MTraits<MF>::d;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.count) return;
  if constexpr (MF == LINEAR2 || MF == LINEAR3) {
    const int i = a.left[q];
    const T cf[4] = {T(a.coef[4 * (size_t)q]), T(a.coef[4 * (size_t)q + 1]), T(a.coef[4 * (size_t)q + 2]), T(a.coef[4 * (size_t)q + 3])};
#pragma unroll
    for (int c = 0; c < d; c++) {
      const T p1 = a.pose[(size_t)c * a.stride + i], p2 = a.pose[(size_t)c * a.stride + i + 1];
      const T v1 = a.vel[(size_t)c * a.stride + i], v2 = a.vel[(size_t)c * a.stride + i + 1];
      a.out[(size_t)q * d + c] = cf[0] * p1 + cf[1] * v1 + cf[2] * p2 + cf[3] * v2;
    }
    if (a.out_H) {
      T *oh = a.out_H + (size_t)q * 4 * d * d;
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int r = 0; r < d; r++)
#pragma unroll
          for (int c = 0; c < d; c++) oh[(m * d + r) * d + c] = (r == c) ? cf[m] : T(0);
    }
  }
}

// getBodyCentricVb / getBodyCentricVs (gpslam/gp/Pose3utils.cpp:17-24; Barfoot14tro eq. 25), batched: thread per pose pair.
//   which 0: Vb = Logmap(pose1^-1 pose2) / dt      which 1: Vs = Logmap(pose2 pose1^-1) / dt
template <typename T>
__global__ void __launch_bounds__(128) k_body_velocity(const double *p1, const double *p2, const double *dt, int count, int which, double *out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= count) return;
  T a[12], b[12];
#pragma unroll
  for (int k = 0; k < 12; k++) { a[k] = T(p1[(size_t)q * 12 + k]); b[k] = T(p2[(size_t)q * 12 + k]); }
  const SE3<T> A = as_se3(a), Bm = as_se3(b);
  const SE3<T> h = which ? se3_compose(Bm, se3_inverse(A)) : se3_between(A, Bm);
  const V6<T> r = se3_log(h);
  const T s = T(1) / T(dt[q]);
  double *o = out + (size_t)q * 6;
  o[0] = s * r.w.x; o[1] = s * r.w.y; o[2] = s * r.w.z; o[3] = s * r.v.x; o[4] = s * r.v.y; o[5] = s * r.v.z;
}

// ------------------------------------------------------------------ K4: partitioned block Gauss-Jordan




template <typename T> struct FwdArgs {
  T *blk;            // n records of this level, eliminated in place
  const T *add;      // n addend records [RD | Rg] or null (level 0)
  T *up_blk;         // records of the next level (one per chunk)
  T *up_add;         // addends of the next level (nchunks + 1)
  int n, m, R;
  int no_sep;        // 1: top level, a single chunk with no separator (plain sequential elimination)
  int last_has_right;// the last chunk has a right separator outside this level (next rank)
  const T *remote_add; // [RD | Rg] already owed to that outside separator by lower levels / the assembly, or null
  T lambda;          // LM damping added to the diagonal of D while loading (level 0 only)
  int *flag;         // set to 1 if a pivot is not positive
  // k_fused_level0 only.  tail = 1: the wave's four chunk separators are reduced to the first of them at the end of the
  // kernel (two sub-levels of cyclic reduction, cr_step.hpp) -- the level of groups of four that upper.hip would otherwise
  // run as a launch of its own.  up_blk / up_add then belong to the level ABOVE that one (one record per workgroup), and
  // the factor records of the three eliminated separators go to l1_blk (the records of the level in between).
  T *l1_blk;
  int tail;
};

// One wave per chunk.  Panel columns: [ D~ (B) | O^T (B) | F (B) | rhs (R) ], one column per lane.
// Block j:  D~_j x_j + O_j^T x_{j+1} + F_j x_sep = g~_j.  Gauss-Jordan on D~_j turns the other columns into
// U_j = D~^-1 O_j^T, V_j = D~^-1 F_j, Y_j = D~^-1 g~_j (stored in place for the back-substitution) and
//   D~_{j+1} = D_{j+1} - O_j U_j,  F_{j+1} = -O_j V_j,  g~_{j+1} = g_{j+1} - O_j Y_j,
//   separator:  D_sep -= F_j^T V_j,  g_sep -= F_j^T Y_j.
// The lanes that held O^T become the D~ lanes of the next block (roles swap), so nothing moves.
// FAST (4B + 2R <= 64): the separator sums live in B + R otherwise idle lanes ("A lanes") and are formed by the
// very same instruction stream as the next-block update -- every lane executes  nxt -= Mat * col, the update lanes
// with Mat = O_j and their own column, the A lanes with Mat = F_j^T and a V_j / Y_j column fetched from LDS --
// which removes a whole B x B multiply-accumulate pass per block and keeps the live state at two B-vectors per lane.
template <typename T, int B, bool FAST>
__global__ void __launch_bounds__(64, 4) k_chunk_forward(FwdArgs<T> a) {
  const int R = a.R;
  const int BS = 2 * B * B + B * R;
  const int AS = B * B + B * R;
  const int c = blockIdx.x;
  const int s = c * a.m;
  const int e = min(s + a.m, a.n);
  const int lane = threadIdx.x;
  const bool has_sep = !a.no_sep;
  const bool right_exists = (e < a.n) || (a.last_has_right != 0);
  // FAST: the eliminated record [V_j | U_j | Y_j] is laid out in LDS exactly as it goes to memory: the A lanes take their
  // V / Y operands from there, and the wave writes it back as contiguous 16-byte pieces (3 wave stores per Pose3 block
  // instead of 6 stores of 16-byte fragments at a 96-byte stride)
  constexpr int kRecLen = FAST ? 2 * B * B + B * ((64 - 4 * B) / 2) : 2;
  __shared__ __attribute__((aligned(16))) T ldsM[2 * B * B];   // [O_j | F_j]: one array, so that Mat below is an offset
  T *const ldsO = ldsM, *const ldsF = ldsM + B * B;
  __shared__ __attribute__((aligned(16))) T ldsRec[kRecLen];
  if (FAST && a.no_sep) {   // no spike columns at the top level: keep the V part of the stored records defined
    for (int q = threadIdx.x; q < B * B; q += 64) ldsRec[q] = T(0);
  }
  int dbase = 0, obase = B;
  const int cF = lane - 2 * B;
  const bool isF = has_sep && cF >= 0 && cF < B;
  const int cR = lane - 3 * B;
  const bool isR = cR >= 0 && cR < R;
  const int cA = lane - (3 * B + R);                      // < B: column of the separator's D; >= B: rhs column
  const bool isA = FAST && has_sep && cA >= 0 && cA < B + R;
  T col[B];
  T nxt[B];                 // update lanes: operand of block j+1;  A lanes: minus the separator sums (persistent)
  T acc[FAST ? 1 : B];      // !FAST: separator sums in the F / rhs lanes
#pragma unroll
  for (int k = 0; k < B; k++) { col[k] = T(0); nxt[k] = T(0); }
#pragma unroll
  for (int k = 0; k < (FAST ? 1 : B); k++) acc[k] = T(0);

  auto load_D_row = [&](int j, int r, T *out) {
    const T *p = a.blk + (size_t)j * BS + r * B;
#pragma unroll
    for (int k = 0; k < B; k++) out[k] = p[k];
    if (a.add) {
      const T *q = a.add + (size_t)j * AS + r * B;
#pragma unroll
      for (int k = 0; k < B; k++) out[k] += q[k];
    }
#pragma unroll
    for (int k = 0; k < B; k++)
      if (k == r) out[k] += a.lambda;
  };
  auto load_O_row = [&](int j, int r, T *out) {
    const T *p = a.blk + (size_t)j * BS + B * B + r * B;
#pragma unroll
    for (int k = 0; k < B; k++) out[k] = p[k];
  };
  auto load_G_col = [&](int j, int r, T *out) {
    const T *p = a.blk + (size_t)j * BS + 2 * B * B + r * B;
#pragma unroll
    for (int k = 0; k < B; k++) out[k] = p[k];
    if (a.add) {
      const T *q = a.add + (size_t)j * AS + B * B + r * B;
#pragma unroll
      for (int k = 0; k < B; k++) out[k] += q[k];
    }
  };

  const int j0 = has_sep ? s + 1 : s;
  if (isA) {
    // the A lanes start from the separator's own row of D (or rhs column) and subtract the sums from it: the loads
    // fly with the first block's instead of being an exposed round trip at the end (one per hierarchy level)
    if (cA < B) load_D_row(s, cA, nxt);
    else load_G_col(s, cA - B, nxt);
  }
  if (j0 < e) {
    if (lane < B) load_D_row(j0, lane, col);
    else if (lane < 2 * B) load_O_row(j0, lane - B, col);
    else if (isF) {
      const T *p = a.blk + (size_t)s * BS + B * B;  // F_first = O_s (acts on x_sep in row s+1)
#pragma unroll
      for (int k = 0; k < B; k++) col[k] = p[k * B + cF];
    } else if (isR) load_G_col(j0, cR, col);
  }

  // The first block's operands are awaited HERE rather than inside the loop: with loads pending on `col` at the loop
  // entry the compiler's wait-count bookkeeping keeps a (partial) wait for memory at the top of every iteration,
  // which then catches the operand prefetch issued just above it.
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  for (int j = j0; j < e; ++j) {
    const bool last = (j == e - 1);
    const int cD = lane - dbase, cO = lane - obase;
    const bool isD = cD >= 0 && cD < B, isO = cO >= 0 && cO < B;
    // Operands of block j+1, fetched early so that the HBM latency hides under the elimination.  The loads are
    // UNCONDITIONAL (every lane reads 12 doubles from a valid address of its role, or block j again) and neither the
    // addend of an upper level nor the damping is folded in here: a load under a branch merges with the zero of the
    // other path, an add consumes the value, and either makes the compiler wait for the load right where it was
    // issued -- 1.4 us per block step of a chunk that runs alone (measured with s_memtime), i.e. on every upper level.
    T araw[B];
    const bool use_n = !last && (isD || isO || isR);
    const bool use_a = !last && a.add != nullptr && (isO || isR);
    {
      const int jn = last ? j : j + 1;
      const T *pn = a.blk + (size_t)jn * BS + (isD ? B * B + cD * B : isO ? cO * B : isR ? 2 * B * B + cR * B : 0);
      const T *pq = a.add ? a.add + (size_t)jn * AS + (isR ? B * B + cR * B : isO ? cO * B : 0) : pn;
      if (!isA) {
#pragma unroll
        for (int k = 0; k < B; k++) nxt[k] = pn[k];
      }
#pragma unroll
      for (int k = 0; k < B; k++) araw[k] = pq[k];
    }
    if (isO) {
#pragma unroll
      for (int k = 0; k < B; k++) ldsO[cO * B + k] = col[k];
    }
    if (isF) {
#pragma unroll
      for (int k = 0; k < B; k++) ldsF[cF * B + k] = col[k];
    }
    // Gauss-Jordan on the D~ columns; every lane applies the same row operations to its column
    const int db = __builtin_amdgcn_readfirstlane(dbase);
#pragma unroll
    for (int k = 0; k < B; k++) {
      // the whole pivot column goes to SGPRs first, then the row operations: back-to-back v_readlane / v_fma pairs
      // on one SGPR pair cost a hazard nop each and serialise on the write-after-read of that pair
      const T p = lane_bcast(col[k], db + k);
      T mlt[B];
#pragma unroll
      for (int i = 0; i < B; i++) mlt[i] = (i != k) ? lane_bcast(col[i], db + k) : T(0);
      if (!(p > T(0)) && lane == 0) *a.flag = 1;
      const T rowk = col[k] * fast_rcp(p);
#pragma unroll
      for (int i = 0; i < B; i++)
        if (i != k) col[i] -= mlt[i] * rowk;
      col[k] = rowk;
    }
    T *bp = a.blk + (size_t)j * BS;
    T *rp = FAST ? ldsRec : bp;                                       // where this block's factors are assembled
    if (isO) {
#pragma unroll
      for (int k = 0; k < B; k++) rp[B * B + cO * B + k] = col[k];  // U_j, column cO
    } else if (isF) {
#pragma unroll
      for (int k = 0; k < B; k++) rp[cF * B + k] = col[k];          // V_j, column cF
    } else if (isR) {
#pragma unroll
      for (int k = 0; k < B; k++) rp[2 * B * B + cR * B + k] = col[k];  // Y_j
    }
    wave_lds_sync();
    if (FAST) {
      typedef T V2 __attribute__((ext_vector_type(2)));
      const V2 *src = reinterpret_cast<const V2 *>(ldsRec);
      V2 *dst = reinterpret_cast<V2 *>(bp);
      for (int q = lane; q < BS / 2; q += 64) dst[q] = src[q];
    }
    if (!FAST && has_sep && (isF || isR)) {   // wide borders: separator sums in a pass of their own
#pragma unroll
      for (int q = 0; q < B; q++) {
        T sacc = T(0);
#pragma unroll
        for (int k = 0; k < B; k++) sacc += ldsF[q * B + k] * col[k];
        acc[q] += sacc;
      }
    }
    // the fetched operands have landed by now: lanes without an operand start from zero, addend and damping join in
    // the summation order of the unfused form (the A lanes keep their running sums)
    if (!isA) {
#pragma unroll
      for (int k = 0; k < B; k++) {
        T v = use_n ? nxt[k] : T(0);
        v += use_a ? araw[k] : T(0);
        v += (use_n && isO && k == cO) ? a.lambda : T(0);
        nxt[k] = v;
      }
    }
    // one B x B product per lane:  nxt -= Mat * col
    const int moff = isA ? B * B : 0;
    if (isA) {
      const T *vp = ldsRec + (cA < B ? cA * B : 2 * B * B + (cA - B) * B);   // column of V_j, or of Y_j
#pragma unroll
      for (int k = 0; k < B; k++) col[k] = vp[k];
    } else if (!(isO || isF || isR)) {
#pragma unroll
      for (int k = 0; k < B; k++) col[k] = T(0);     // D lanes (and spare lanes) take the operand unchanged
    }
    {
      // rows of Mat are wave-uniform (broadcast) 16-byte LDS reads; row r + 1 is in flight while row r is used, so
      // the loop waits on LDS once per row instead of once per operand pair
      typedef T V2 __attribute__((ext_vector_type(2)));
      const V2 *M2 = reinterpret_cast<const V2 *>(ldsM + moff);
      V2 cur[B / 2], nx[B / 2];
#pragma unroll
      for (int k = 0; k < B / 2; k++) cur[k] = M2[k];
#pragma unroll
      for (int r = 0; r < B; r++) {
        if (r + 1 < B) {
#pragma unroll
          for (int k = 0; k < B / 2; k++) nx[k] = M2[(r + 1) * (B / 2) + k];
        }
        T sacc = T(0);
#pragma unroll
        for (int k = 0; k < B / 2; k++) {
          sacc += cur[k].x * col[2 * k];
          sacc += cur[k].y * col[2 * k + 1];
        }
        nxt[r] -= sacc;
#pragma unroll
        for (int k = 0; k < B / 2; k++) cur[k] = nx[k];
      }
    }
    if (!last) {
      if (!isA) {
#pragma unroll
        for (int r = 0; r < B; r++) col[r] = nxt[r];
      }
      const int tswap = dbase; dbase = obase; obase = tswap;
    } else if (right_exists && has_sep) {
      T *ua = a.up_add + (size_t)(c + 1) * AS;
      const T *ra = (e == a.n) ? a.remote_add : nullptr;   // carry what is already owed to the outside separator
      if (isO) {
#pragma unroll
        for (int k = 0; k < B; k++) ua[cO * B + k] = (ra ? ra[cO * B + k] : T(0)) + nxt[k];              // -O U  (symmetric)
      } else if (isR) {
#pragma unroll
        for (int k = 0; k < B; k++) ua[B * B + cR * B + k] = (ra ? ra[B * B + cR * B + k] : T(0)) + nxt[k];      // -O Y
      } else if (isF) {
        T *uo = a.up_blk + (size_t)c * BS + B * B;
#pragma unroll
        for (int r = 0; r < B; r++) uo[r * B + cF] = nxt[r];             // C = -O V, couples sep c -> sep c+1
      }
    }
    wave_lds_sync();
  }

  if (has_sep) {
    T *ub = a.up_blk + (size_t)c * BS;
    // separator block of the next level: D_sep - sum F^T V (row = column by symmetry), g_sep - sum F^T Y
    const bool wD = FAST ? (isA && cA < B) : isF;
    const bool wG = FAST ? (isA && cA >= B) : isR;
    const int rD = FAST ? cA : cF, rG = FAST ? cA - B : cR;
    if (wD) {
      T dr[B];
      if (!FAST) load_D_row(s, rD, dr);
#pragma unroll
      for (int k = 0; k < B; k++) ub[rD * B + k] = FAST ? nxt[k] : dr[k] - acc[FAST ? 0 : k];
    } else if (wG) {
      T gr[B];
      if (!FAST) load_G_col(s, rG, gr);
#pragma unroll
      for (int k = 0; k < B; k++) ub[2 * B * B + rG * B + k] = FAST ? nxt[k] : gr[k] - acc[FAST ? 0 : k];
    }
    if (j0 >= e) {  // chunk without interior: the separator keeps its original coupling
      if (lane < B) {
        T orow[B];
        load_O_row(s, lane, orow);
#pragma unroll
        for (int k = 0; k < B; k++) ub[B * B + lane * B + k] = right_exists ? orow[k] : T(0);
        if (right_exists) {
          T *ua = a.up_add + (size_t)(c + 1) * AS;
          const T *ra = (e == a.n) ? a.remote_add : nullptr;
#pragma unroll
          for (int k = 0; k < B; k++) ua[lane * B + k] = ra ? ra[lane * B + k] : T(0);
        }
      }
      if (isR && right_exists) {
        T *ua = a.up_add + (size_t)(c + 1) * AS;
        const T *ra = (e == a.n) ? a.remote_add : nullptr;
#pragma unroll
        for (int k = 0; k < B; k++) ua[B * B + cR * B + k] = ra ? ra[B * B + cR * B + k] : T(0);
      }
    } else if (!right_exists) {
      if (lane < B) {
#pragma unroll
        for (int k = 0; k < B; k++) ub[B * B + lane * B + k] = T(0);
      }
    }
  }
}

// ---------------------------------------------------------------- the arguments of k_fused_level0 (level0.hpp)
//
// TR: type of the Jacobian row tables (float on fp32 handles -- GPSLAM_FP32 --, whose accumulation, normal equations and
// elimination stay fp64: the rows are widened as they leave the ring)
template <typename T, typename TR = T> struct FusedArgs {
  FwdArgs<T> f;           // level-0 arguments of the elimination (blk: where the factors [V | U | Y] go)
  const int *rowptr;      // full-width rows of left state s: [rowptr[s], rowptr[s+1])
  const TR *rowLR, *rowE; // M x 24, M
  const int *crowptr;     // compact rows
  const TR *rowC, *rowCE; // Mc x 12, Mc
  const T *rowI = nullptr;       // k_fused_level0<4>: the interpolated measurement rows as 16-double lines (kIRow*), indexed by irowptr
  const int *irowptr = nullptr;  // n + 2 entries, like rowptr, counting only those rows (the GP priors have none: they are records)
  const T *gps;           // structured GP-prior records (kGpsLen each, see GpArgs::gps) or null: the GP rows are in rowLR
  int gp_count;           // number of records; record gp_count is all zeros (states without a GP prior read it)
  const T *brec;          // BetweenFactor<Pose3> records (kBtw*; K1 wrote no compact rows for them) or null (ST variants only)
  const int *btwidx;      // n + 2 entries: record of the between factor whose left state is s, or -1
  int btw_count;          // number of records; record btw_count is all zeros
  const int *gpidx;       // n + 2 entries: record of the GP prior whose left state is s, or -1
  int odd_rows;           // the structured chain has other full-width rows as well: 1 = a few (k_fused_level0<2>), 2 = many (<3>: a ring)
  int u_diag;             // Ud is diagonal (SE(3) records: k_fused_level0<1, double, 12, true>)
  const T *Ud;            // chol_upper(Qc^-1), row-major 6 x 6, in device memory: the structured velocity columns are multiples of its rows
  int *simd_cnt = nullptr;       // round 6 (role swap): wave-0 count per SIMD of the chip (8192 ints, zero between launches), or null
  T *gsave, *gsave2;      // Levenberg-Marquardt: the gradient g = -J^T e per state (gsave) and, for a chunk's separator, the part of
                          // it that the PREVIOUS chunk's last rows contribute (gsave2; zero elsewhere); null: not wanted
#ifdef GPS_TRACE_FUSED
  unsigned long long *trace = nullptr;   // debug builds only: 64 stamps per wave (scripts/trace_fused.py)
#endif
};

template <typename T> struct BwdArgs {
  const T *blk;   // eliminated records of this level
  T *x;           // n x R x B solutions of this level (+ one slot for the neighbour rank's separator)
  const T *xup;   // solutions of the next level (separators) or null at the top
  int n, m, R, no_sep, last_has_right;
  // k_chunk_backward_rows only (round 4): the level above is the level of groups of four that k_fused_level0 reduced in its tail --
  // a wave's four chunks ARE one such group, so the wave back-substitutes the group itself (l1_blk: that level's factor records,
  // l1_xup: the solutions of the group's first block and of the next group's, one level further up) instead of a launch of
  // k_multi_backward<B, 4> writing xup for it.  Null: xup holds the separators' solutions.
  const T *l1_blk = nullptr, *l1_xup = nullptr;
  int l1_n = 0;   // blocks of that level (= chunks of this one)
};

// The launchers of the level-0 forms that exist for fp64 records only (hand-written 64-bit DPP row layout).  level0.hip defines them
// and is the one unit that compiles their kernels (level0.hpp); both precision halves call them (api_impl.inc).  cen: the handle's
// launch census (GPSLAM_CENSUS_*), written at the launch statement from the branch taken.  launch_fused_k: k_fused_level0<sv, TR, b, dg>
// (fp32 row tables reach <0, float> alone); ea / eb != null: the launch carries its own start / stop events (a timed iteration)
void launch_fused_k(int32_t *cen, int b, int sv, bool dg, const FusedArgs<double, double> &u, int grid, hipStream_t st, hipEvent_t ea = nullptr, hipEvent_t eb = nullptr);
void launch_fused_k(int32_t *cen, int b, int sv, bool dg, const FusedArgs<double, float> &u, int grid, hipStream_t st, hipEvent_t ea = nullptr, hipEvent_t eb = nullptr);
void launch_rows_k(int32_t *cen, int b, const FwdArgs<double> &a, int grid, hipStream_t st);
void launch_bwd_rows_k(int32_t *cen, int b, const BwdArgs<double> &a, int grid, hipStream_t st);

// x_j = Y_j - U_j x_{j+1} - V_j x_sep, right to left through the chunk.  Lane (k, rr) owns component k of the rhs
// columns rr, rr + RG, ...  The pass is pure streaming (2400 B of factors per 24 FMAs on 12 lanes for Pose3), so it
// lives or dies by how the factors arrive: the wave fetches each record [V | U | Y] as contiguous 16-byte pieces
// (NP wave loads of 1 KiB instead of 25 loads of 96 useful bytes), PFB records ahead in a register ring, and hands
// them to the consuming lanes through LDS.  NP = 16-byte pieces per lane per record: 3 covers R <= 8 for B = 12.
template <typename T, int B, int NP>
__global__ void __launch_bounds__(64) k_chunk_backward(BwdArgs<T> a) {
  const int R = a.R;
  const int BS = 2 * B * B + B * R;
  const int c = blockIdx.x;
  const int s = c * a.m;
  const int e = min(s + a.m, a.n);
  const int lane = threadIdx.x;
  const bool has_sep = !a.no_sep;
  const bool right_exists = has_sep && ((e < a.n) || (a.last_has_right != 0));
  constexpr int RG = 64 / B;
  constexpr int PFB = 4;   // records in flight (round 3: 3 -> 4 with the longer chunks of large chains: 485 -> 452 us at 1e6 states; 6: 510 us)
  const int rr = lane / B, k = lane - rr * B;
  const bool active = rr < RG;
  typedef T V2 __attribute__((ext_vector_type(2)));
  __shared__ T xs[kMaxRhs * B];
  __shared__ T xa[kMaxRhs * B];
  __shared__ T xb[kMaxRhs * B];
  __shared__ __attribute__((aligned(16))) T rec[NP * 128];      // one record [V | U | Y]
  for (int idx = lane; idx < R * B; idx += 64) {
    xs[idx] = has_sep ? a.xup[(size_t)c * R * B + idx] : T(0);
    xa[idx] = right_exists ? a.xup[(size_t)(c + 1) * R * B + idx] : T(0);
  }
  wave_lds_sync();
  if (has_sep)
    for (int idx = lane; idx < R * B; idx += 64) a.x[(size_t)s * R * B + idx] = xs[idx];
  // the right separator of the last chunk lives on the next rank: park its solution in the extra slot x[n] so
  // that the level below finds it where it expects the solution of "separator n"
  if (right_exists && e == a.n)
    for (int idx = lane; idx < R * B; idx += 64) a.x[(size_t)a.n * R * B + idx] = xa[idx];
  const int j0 = has_sep ? s + 1 : s;
  const int pieces = BS / 2;                                      // BS is even (B is)
  V2 ring[PFB][NP];
  // The record loads are UNCONDITIONAL (record index clamped into the chunk, piece index into the record): a load under
  // a branch -- or a ring slot that is only sometimes refilled -- makes the compiler's wait-count bookkeeping give up
  // and drain vmcnt to zero at every step, which turns the 3-deep prefetch into none at all and additionally waits
  // for the x stores (2.6 us per block step measured, a full memory round trip).  Steps past the chunk's first
  // interior record recompute harmlessly; only their x store is masked.
  const int jlo = min(j0, e - 1);
  auto arm = [&](int u, int j) {
    const V2 *src = reinterpret_cast<const V2 *>(a.blk + (size_t)max(j, jlo) * BS);
#pragma unroll
    for (int p = 0; p < NP; p++) ring[u][p] = src[min(lane + 64 * p, pieces - 1)];
  };
  if (j0 < e) {
#pragma unroll
    for (int u = 0; u < PFB; u++) arm(u, e - 1 - u);
  }
  int ping = 0;
  for (int base = e - 1; base >= j0; base -= PFB) {
#pragma unroll
    for (int u = 0; u < PFB; u++) {
      const int j = base - u;
      V2 *rv = reinterpret_cast<V2 *>(rec);
#pragma unroll
      for (int p = 0; p < NP; p++) rv[lane + 64 * p] = ring[u][p];
      arm(u, j - PFB);
      wave_lds_sync();
      const T *cur = ping ? xb : xa;
      T *nx = ping ? xa : xb;
      if (active) {
        T Ur[B], Vr[B];
#pragma unroll
        for (int q = 0; q < B; q++) { Ur[q] = rec[B * B + q * B + k]; Vr[q] = has_sep ? rec[q * B + k] : T(0); }
        for (int r = rr; r < R; r += RG) {
          T v = rec[2 * B * B + r * B + k];
#pragma unroll
          for (int q = 0; q < B; q++) v -= Ur[q] * cur[r * B + q] + Vr[q] * xs[r * B + q];
          nx[r * B + k] = v;
          if (j >= j0) a.x[(size_t)j * R * B + r * B + k] = v;
        }
      }
      wave_lds_sync();
      ping ^= 1;
    }
  }
}

// ------------------------------------------------------------------ segment sharding: reduced interface system

// Every rank contributes one record [D | C | G | RD | Rg] (BS + AS values): its separator block (first state) after
// the local elimination, the coupling C to the next rank's separator and the addend it owes that separator.
// top[r] = [D_r + RD_{r-1} | C_r | G_r + Rg_{r-1}]
template <typename T> __global__ void __launch_bounds__(256) k_iface_build(const T *rec, int P, int B, int R, T *top) {
  const int BS = 2 * B * B + B * R, AS = B * B + B * R, RS = BS + AS;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * BS) return;
  const int r = i / BS, k = i - r * BS;
  T v = rec[(size_t)r * RS + k];
  if (r > 0) {
    const T *pa = rec + (size_t)(r - 1) * RS + BS;
    if (k < B * B) v += pa[k];
    else if (k >= 2 * B * B) v += pa[B * B + (k - 2 * B * B)];
  }
  if (r == P - 1 && k >= B * B && k < 2 * B * B) v = T(0);   // no coupling beyond the last rank
  top[i] = v;
}

// ------------------------------------------------------------------ K6: retract

template <typename T> struct RetractArgs {
  double *pose, *vel;   // the state is fp64 whatever T is: the update is applied in fp64
  int stride, N, R, chart;
  int first;        // first state to update (the halo state of a segment is updated by its own launch)
  const T *x;       // N x R x b, column 0 = delta (indexed from `first`)
  T *partial;       // per-block max |delta|
  const int *flag;  // non-SPD flag of the elimination: when set the states are left untouched (GTSAM throws
                    // IndeterminantLinearSystemException before Values::retract), only |delta|_inf is reported
  // deferred reduction (round 3): the per-block error sums of this iteration's linearisation, summed by one extra
  // workgroup at the end of the grid instead of by a launch of their own right behind the linearisation
  const double *red_in = nullptr;
  int red_n = 0;
  double *red_out = nullptr;
};

template <typename T, int MF>
__global__ void __launch_bounds__(128) k_retract(RetractArgs<T> a) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd, b = 2 * d;
  if (a.red_in != nullptr && blockIdx.x == gridDim.x - 1) {     // the extra workgroup: pending error sum, fixed order
    const double acc = strided_fold<double, 128>(a.red_in, a.red_n, 0);
    const double r = block_sum(acc);
    if (threadIdx.x == 0) *a.red_out = r;
    return;
  }
  const int li = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = a.first + li;
  T mx = T(0);
  if (li < a.N) {
    const T *dl = a.x + (size_t)li * a.R * b;
    double dlt[b], x[pd], out[pd];
#pragma unroll
    for (int k = 0; k < b; k++) { dlt[k] = (double)dl[k]; mx = fmax(mx, abs_or_inf(dl[k])); }
    if (!(a.flag && *a.flag)) {
#pragma unroll
      for (int k = 0; k < pd; k++) x[k] = a.pose[(size_t)k * a.stride + i];
      PoseFactors<double, MF, false>::retract(x, dlt, a.chart, out);
#pragma unroll
      for (int k = 0; k < pd; k++) a.pose[(size_t)k * a.stride + i] = out[k];
#pragma unroll
      for (int k = 0; k < d; k++) a.vel[(size_t)k * a.stride + i] += dlt[d + k];
    }
  }
  const T r = block_max(mx);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = r;
}

}  // namespace gps
