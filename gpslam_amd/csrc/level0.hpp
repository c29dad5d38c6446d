// level0.hpp -- the level-0 forms that exist for fp64 solver records only, on 16-lane DPP rows: k_chunk_forward_rows,
// k_fused_level0 (K3 inside K4) and k_chunk_backward_rows.  level0.hip is the one translation unit that includes this file: it
// compiles every form once and defines the launchers kernels.hpp declares (launch_rows_k, launch_fused_k, launch_bwd_rows_k).
// The argument structs (FwdArgs, FusedArgs, BwdArgs) are kernels.hpp's: the callers fill them without seeing a kernel.
#pragma once

#include "kernels.hpp"

namespace gps {

// ---------------------------------------------------------------- row-layout forward elimination (Pose3, R = 1)
//
// Same elimination as k_chunk_forward, same records in and out, different mapping: FOUR chunks per wave, one per
// 16-lane DPP row, lane r < 12 of a row holding ROW r of the panel [ D~_j | O_j^T | F_j | g~_j ].  The multipliers
// D~[r][k] of a Gauss-Jordan step are then lane-local and only the pivot row travels -- by `v_mov_b32_dpp
// row_newbcast:k` (full VALU rate, no SGPR round trip) instead of a v_readlane per multiplier.  The updates
//   D~_{j+1} = D_{j+1} - O_j U_j,  F_{j+1} = -O_j V_j,  g~_{j+1} = g_{j+1} - O_j Y_j
// take row r of O_j as local scalars against broadcast rows of U_j / V_j / Y_j; the separator sums need F_j^T,
// which is carried alongside as G_j = F_j^T with  G_{j+1} = -G_j U_j  (V_j^T = G_j D~_j^-1 by symmetry):
//   D_sep -= G_j V_j,  g_sep -= G_j Y_j.
// Records enter and leave as contiguous 16-byte pieces through a per-row LDS image (which also provides the
// transposed reads of O).  ~660 VALU instructions per chunk-step against ~830 (288 of them v_readlane) before.
// Round 3: the block size is a template parameter (12: SE(3); 6: SE(2), SO(3), 3-D linear; 4: 2-D linear) -- the planar /
// rotation chains had kept the column-layout kernel (k_chunk_forward), at 1.7 TB/s of record traffic where this one is bound
// by it.
template <int B>
__global__ void __launch_bounds__(64, 2) k_chunk_forward_rows(FwdArgs<double> a) {
  constexpr int BS = 2 * B * B + B, AS = B * B + B;   // R == 1
  constexpr int NPC = BS / 2;                                  // 16-byte pieces of a record
  constexpr int NV = (NPC + 15) / 16;                          // pieces per lane of a 16-lane row
  typedef double V2 __attribute__((ext_vector_type(2)));
  const int lane = threadIdx.x, grp = lane >> 4, r = lane & 15;
  const int c = blockIdx.x * 4 + grp;
  const int nch = (a.n + a.m - 1) / a.m;
  const bool valid = c < nch;
  const int s = valid ? c * a.m : 0;
  const int e = valid ? min(s + a.m, a.n) : 0;
  const int j0 = s + 1;
  const bool rowlane = r < B;
  const int rr = rowlane ? r : 0;                              // idle lanes shadow row 0 (they never store)
  const bool right_exists = (e < a.n) || (a.last_has_right != 0);
  const bool has_int = valid && j0 < e;
  const double lambda = a.lambda;
  __shared__ __attribute__((aligned(16))) double L[4 * BS];   // one record image per 16-lane row
  // Every LDS access below is  L[opaque per-lane offset + compile-time constant]: left to itself the compiler derives the
  // row / column / piece addresses from one another by strength reduction and ends up with a dozen VGPRs holding the
  // same address (40 VGPRs, which spilled -- and every scratch reload drains vmcnt, i.e. waits for the factor stores)
  int ro = grp * BS + rr * B;     // row r:      L[ro + k]
  int co = grp * BS + rr;         // column r:   L[co + k * B]
  int po = grp * BS + 2 * r;      // 16-byte piece q * 16 + r of the image: L[po + 32 * q]
  int dg = grp * BS + rr * B + rr;
  asm volatile("" : "+v"(ro), "+v"(co), "+v"(po), "+v"(dg));

  // record j as 16-byte pieces, unconditionally (clamped): whether it exists is applied when it is consumed
  auto load_rec = [&](int j, V2 *v) {
    const V2 *src = reinterpret_cast<const V2 *>(a.blk + (size_t)min(max(j, 0), a.n - 1) * BS);
#pragma unroll
    for (int t = 0; t < NV; t++) v[t] = src[min(t * 16 + r, NPC - 1)];
  };
  auto put_rec = [&](const V2 *v, bool ok) {
#pragma unroll
    for (int t = 0; t < NV; t++) {
      const int idx = t * 16 + r;
      V2 w = v[t];
      if (!ok) { w.x = 0.0; w.y = 0.0; }
      if (idx < NPC) *reinterpret_cast<V2 *>(&L[po + 32 * t]) = w;
    }
  };
  auto add_lambda = [&](bool ok) {
    if (lambda != 0.0) {
      if (rowlane && ok) L[dg] += lambda;
      wave_lds_sync();
    }
  };

  V2 pa[NV], pb[NV];
  load_rec(s, pa);
  load_rec(j0, pb);
  double Dr[B], Or[B], Fr[B], Gr[B], Ar[B];
  double gr, as_;
  put_rec(pa, valid);
  wave_lds_sync();
  add_lambda(valid);
#pragma unroll
  for (int k = 0; k < B; k++) {
    Ar[k] = L[ro + k];                       // row r of D_sep
    Fr[k] = L[ro + B * B + k];               // F_{s+1} = O_s: row r
    Gr[k] = L[co + B * B + k * B];           // G_{s+1} = O_s^T: row r
  }
  as_ = L[co + 2 * B * B];
  wave_lds_sync();
  put_rec(pb, has_int);
  wave_lds_sync();
  add_lambda(has_int);
#pragma unroll
  for (int k = 0; k < B; k++) {
    Dr[k] = L[ro + k];                       // row r of D_j
    Or[k] = L[co + B * B + k * B];           // row r of O_j^T
  }
  gr = L[co + 2 * B * B];
  // (the image of record j stays in LDS through the elimination: row r of O_j is fetched from it afterwards, which
  //  keeps 24 VGPRs free while the prefetched record j + 1 occupies 40)

  if (valid && !has_int && rowlane) {        // chunk without interior: the separator keeps its original coupling
    double *ub = a.up_blk + (size_t)c * BS;
#pragma unroll
    for (int k = 0; k < B; k++) {
      ub[r * B + k] = Ar[k];
      ub[B * B + r * B + k] = right_exists ? Fr[k] : 0.0;
    }
    ub[2 * B * B + r] = as_;
    if (right_exists) {
      double *ua = a.up_add + (size_t)(c + 1) * AS;
      const double *ra = (e == a.n) ? a.remote_add : nullptr;
#pragma unroll
      for (int k = 0; k < B; k++) ua[r * B + k] = ra ? ra[r * B + k] : 0.0;
      ua[B * B + r] = ra ? ra[B * B + r] : 0.0;
    }
  }

  // lane 0 belongs to the wave's first chunk, which is never shorter than the others
  const int steps = __builtin_amdgcn_readfirstlane(max(e - j0, 0));
  for (int t = 0; t < steps; t++) {
    const int j = j0 + t;
    const bool live = j < e, lastb = (j == e - 1), nextlive = (j + 1 < e);
    V2 pf[NV];
    load_rec(j + 1, pf);                     // record j + 1 flies under the elimination of block j
    __builtin_amdgcn_sched_barrier(0);
    // Gauss-Jordan on D~_j by row operations; the pivot row stays unscaled until the end (scaling commutes)
    double invs = 1.0;
    static_for<0, B>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      const double piv = row_bcast<k>(Dr[k]);
      const double inv = fast_rcp(piv);
      const bool isk = (r == k);
      invs = isk ? inv : invs;
      const double nmp = isk ? 0.0 : -(Dr[k] * inv);
      // row r -= (D~[r][k] / pivot) * row k, the pivot row fused into the multiply-add (fmac_self*): of D~ only the columns
      // right of the pivot still matter, in blocks of four (entries at or left of the pivot inside a block become garbage
      // that nothing reads again)
      if constexpr (B == 12) {
        if (k < 3) fmac_self4<k>(Dr, nmp);
        if (k < 7) fmac_self4<k>(Dr + 4, nmp);
        if (k < 11) fmac_self4<k>(Dr + 8, nmp);
      } else {
        fmac_self_n<k, B>(Dr, nmp);
      }
      fmac_self_n<k, B>(Or, nmp);
      fmac_self_n<k, B>(Fr, nmp);
      fmac_self1<k>(gr, nmp);
    });
    // a pivot that is not positive (or not a number) leaves a reciprocal that is not positive in its own lane: one test per
    // block step instead of one per pivot (lanes without a row keep 1)
    if (!(invs > 0.0) && live) *a.flag = 1;
    __builtin_amdgcn_sched_barrier(0);
    double Ol[B];
#pragma unroll
    for (int k = 0; k < B; k++) Ol[k] = L[ro + B * B + k];          // row r of O_j, from the image of record j
#pragma unroll
    for (int k = 0; k < B; k++) { Or[k] *= invs; Fr[k] *= invs; }   // U_j, V_j: row r
    gr *= invs;                                                      // Y_j
    wave_lds_sync();
    if (rowlane) {
#pragma unroll
      for (int k = 0; k < B; k++) {
        L[co + k * B] = Fr[k];               // the stored record is column-major [V | U | Y]
        L[co + B * B + k * B] = Or[k];
      }
      L[co + 2 * B * B] = gr;
    }
    wave_lds_sync();
    if (live) {
      V2 *dst = reinterpret_cast<V2 *>(a.blk + (size_t)j * BS);
#pragma unroll
      for (int q = 0; q < NV; q++) {
        const int idx = q * 16 + r;
        if (idx < NPC) dst[idx] = *reinterpret_cast<const V2 *>(&L[po + 32 * q]);
      }
    }
    wave_lds_sync();
    put_rec(pf, nextlive);                   // zeros after the chunk's last block: the products then are the addends
    wave_lds_sync();
    add_lambda(nextlive);
    double Dn[B], Fn[B], Gn[B], gn;
#pragma unroll
    for (int k = 0; k < B; k++) { Dn[k] = L[ro + k]; Gn[k] = 0.0; }
    gn = L[co + 2 * B * B];
    __builtin_amdgcn_sched_barrier(0);
    // two passes, so that at most seven 12-vectors are live: rows of U_j first (O_j^T is dead afterwards) ...
    static_for<0, B>([&](auto ii) {
      constexpr int i = decltype(ii)::value;
      const double ol = Ol[i], gg = Gr[i];          // subtracted: the negation is the instructions' source modifier
      fmac_bcast_n<i, B, true>(Dn, Or, ol);     // D~_{j+1} -= O_j[r][i] * (row i of U_j)
      fmac_bcast_n<i, B, true>(Gn, Or, gg);     // G_{j+1}  -= G_j[r][i] * (row i of U_j)
      fmac_bcast2<i, true>(gn, as_, gr, ol, gg);
    });
    // (pinned here: the compiler otherwise sinks the G_{j+1} sums below the output branch at the end of the step and
    //  spills all 144 broadcast values to feed them there)
#pragma unroll
    for (int k = 0; k < B; k++) asm volatile("" : "+v"(Gn[k]), "+v"(Dn[k]));
    __builtin_amdgcn_sched_barrier(0);
    // ... then rows of V_j
#pragma unroll
    for (int k = 0; k < B; k++) Fn[k] = 0.0;
    static_for<0, B>([&](auto ii) {
      constexpr int i = decltype(ii)::value;
      const double ol = Ol[i], gg = Gr[i];          // subtracted: the negation is the instructions' source modifier
      fmac_bcast_n<i, B, true>(Fn, Fr, ol);     // F_{j+1} -= O_j[r][i] * (row i of V_j)
      fmac_bcast_n<i, B, true>(Ar, Fr, gg);     // D_sep   -= G_j[r][i] * (row i of V_j)
    });
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < B; k++) asm volatile("" : "+v"(Fn[k]), "+v"(Ar[k]));
#pragma unroll
    for (int k = 0; k < B; k++) {
      Dr[k] = Dn[k]; Fr[k] = Fn[k]; Gr[k] = Gn[k];
      Or[k] = L[co + B * B + k * B];
    }
    gr = gn;
    __builtin_amdgcn_sched_barrier(0);
    if (live && lastb && rowlane) {          // after the chunk's last block the "next block" operands are the addends
      double *ub = a.up_blk + (size_t)c * BS;
#pragma unroll
      for (int k = 0; k < B; k++) {
        ub[r * B + k] = Ar[k];                                 // D_sep - sum G V
        ub[B * B + r * B + k] = right_exists ? Fr[k] : 0.0;   // C = -O V couples separator c to separator c + 1
      }
      ub[2 * B * B + r] = as_;
      if (right_exists) {
        double *ua = a.up_add + (size_t)(c + 1) * AS;
        const double *ra = (e == a.n) ? a.remote_add : nullptr;   // what is already owed to the outside separator
#pragma unroll
        for (int k = 0; k < B; k++) ua[r * B + k] = (ra ? ra[r * B + k] : 0.0) + Dr[k];   // -O U
        ua[B * B + r] = (ra ? ra[B * B + r] : 0.0) + gr;                                    // -O Y
      }
    }
    wave_lds_sync();
  }
}

// ---------------------------------------------------------------- assembly fused into the level-0 elimination
//
// k_fused_level0: a workgroup is TWO waves that share four chunks.  Wave 1 (ASM) forms the records [D_j | O_j | g_j]
// of the chunks' states straight from the row tables -- what k_assemble_ghost does, but chunk by chunk, state after
// state, in the row layout of the elimination: lane r of a 16-lane row accumulates row r of D and O; per Jacobian row
// it loads its own L and R element, gathers the 12 L (then the 12 R) elements of the row with
// `v_mov_b64_dpp row_newbcast:0..11` and adds L[r] L[k] -> D_j, R[r] L[k] -> O_j, R[r] R[k] -> the carry that opens
// D_{j+1}.  Wave 0 (ELIM) is k_chunk_forward_rows with the record images coming from ASM through LDS (two rotating
// images per chunk, one s_barrier per block step) instead of from memory.  The block records [D | O | g] never exist in
// HBM: -240 MB written, -262 MB read per iteration, and k_assemble_ghost's launch is gone.
// Conventions that differ from the unfused pair: a separator's own record holds only its rows' L^T L part -- the
// R^T R of the rows of the state before it (the previous chunk's last state) reaches it as part of the addend that
// chunk sends to the upper level anyway (the "virtual" record after a chunk's last state is [carry | 0 | carry_g]).
#ifdef GPS_TRACE_FUSED
#define GPS_TR(slot) do { if (u.trace && lane == 0) u.trace[((size_t)blockIdx.x * 2 + role) * 64 + (slot)] = wall_clock64(); } while (0)
#define GPS_TRA(slot) do { if (kimg == 13) GPS_TR(slot); } while (0)
#define GPS_TRE(slot) do { if (t == 10) GPS_TR(slot); } while (0)
#else
#define GPS_TR(slot) do { } while (0)
#define GPS_TRA(slot) do { } while (0)
#define GPS_TRE(slot) do { } while (0)
#endif


// ST: every full-width row of the chain belongs to a GP prior and K1 delivers those as structured records (u.gps): the
// full-width row ring is replaced by the record ring (a kernel with both spills: 256 VGPRs + 176 B of scratch, 0.34 ms).
// SV = 2: a structured chain that also has a few other full-width rows (a velocity prior or two): those are fetched where
// they are used, without a ring (the pure variant stays free of that loop's registers: with it the kernel spills again).
// (round 3: the block size is a template parameter -- 12: SE(3), with or without structured GP records; 6: SE(2), SO(3), 3-D linear
// chains, plain rows only)
// DG (round 4; SV = 1, B = 12): U = chol_upper(Qc^-1) is DIAGONAL (an isotropic or diagonal Qc, the common case; the host looks at
// the 36 numbers).  Then row q of the whitened L has, among its six velocity columns, only the one of its own component
// (L's velocity block is [k2 U; -sc U]): D and O need 7 instead of 12 multiply-adds per Jacobian row, and U Z is six products per
// six-vector instead of 21 multiply-adds -- 204 of the assembly wave's ~1170 instructions per block step.  What is skipped are
// products with exact zeros: the same values as the general kernel.
constexpr int kFusedWaves = 2;   // waves per SIMD k_fused_level0 is compiled for (two workgroups' worth: see "Wave priority" below)
// Wave priority inside k_fused_level0 (round 6).  The two waves a SIMD holds belong to two different workgroups, and the
// instruction arbiter serves the OLDER wave first: in a launch of one resident set (1e5 states: 1000 workgroups) the workgroups whose
// waves were placed first run at the speed of a wave that has its SIMD to itself and end at 115 us, those placed second take what is
// left and end at 145-154 us -- the launch lasts as long as the slowest (scripts/trace_fused.py, HW_ID wave slots).  So
// every block step a wave sets its priority to 3 - (step mod 4), so the wave that is BEHIND on its SIMD is the one
// that is served first and the workgroups of a CU advance together: the spread of a CU's workgroups falls from ~30 us to 4 us, the
// launch from 154 to 142-145 us at the same median (132 us: the work is what it was), 1e6 states unchanged (workgroups come and go
// there).  Measured and not kept: one role always first (no gain), a two-step quantum (half the gain), a half-step
// quantum (no better).  Rounds 1-5 set no priority.  HISTORY.md "Round 6" has the tables.
// Which wave of a workgroup eliminates (round 6).  The hardware puts wave 0 of a two-wave workgroup on SIMD a and wave 1
// on sigma(a), sigma the 4-cycle 3 -> 0 -> 2 -> 1 -> 3 (HW_ID of 1000 workgroups, scripts/trace_fused.py); a CU's four workgroups then
// either start on four different SIMDs -- every SIMD holds one wave 0 and one wave 1 -- or two by two on the same pair, and with
// "wave 0 eliminates" two SIMDs of that CU hold two elimination waves (5.4 us per block step instead of 4.8) and two hold two assembly
// waves: 27-76 of the chip's 1024 SIMDs per launch, and their workgroups are the launch's last.  So wave 0 counts
// itself into a per-SIMD word (one returning atomic per workgroup, undone on exit): the SECOND wave 0 of a SIMD trades roles with its
// wave 1, which puts an elimination wave on sigma(a) -- where the first workgroup's assembly wave sits -- and every SIMD of every CU
// holds one wave of each kind.  (Exact for a launch of one resident set, where it matters: 1e5 states.  Where workgroups come and go the
// word counts wave 0s, not elimination waves -- a newcomer next to a workgroup that traded sees the count and trades as well -- and
// the launch's duration does not depend on the placement: 1e6 states 1.27 ms with or without.)
// (block size 12 only: the three-waves-per-SIMD kernel of the d = 3 chains gains nothing at 1e5 states and loses 2 % at 1e6)
// c: progress in half steps (2 t at the top of block step t, 2 t + 1 in its middle); the priority changes at whole steps
template <int B> __device__ __forceinline__ void fused_step_prio(int c) {
  if constexpr (B != 12) return;
  if (c & 1) return;
  const int q = (c >> 1) & 3;
  if (q == 0) __builtin_amdgcn_s_setprio(3);
  else if (q == 1) __builtin_amdgcn_s_setprio(2);
  else if (q == 2) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}
template <int SV, typename TR = double, int B = 12, bool DG = false>
__global__ void __launch_bounds__(128, kFusedWaves) k_fused_level0(FusedArgs<double, TR> u) {
  static_assert(SV == 0 || std::is_same<TR, double>::value, "structured GP records are fp64");
  static_assert(!DG || ((SV == 1 || SV == 3 || SV == 4) && B == 12), "the diagonal-U form belongs to the SE(3) record variants");
  // SV = 3 (round 4): records AND a ring of full-width rows -- SE(3) chains with interpolated measurement factors (GPS, range,
  // projection: a dozen full-width rows per state), which had lost the records to the plain-row kernel
  // SV = 4 (round 5): records AND interpolated measurement rows as 16-double lines (kIRow*): one operand per row and lane, a whole
  // state's dozen rows in flight, the right halves formed here from mu and the record's X / F X columns
  constexpr bool ST = SV != 0, ODD = SV >= 2, ORING = SV == 3, IROW = SV == 4;
  static_assert(!IROW || B == 12, "interpolated rows are an SE(3) form");
  // ST12: SE(3) records (kGps*, kBtw*: the assembly wave forms the columns, no full-width row ring);  ST6 (round 4): the d = 3
  // records (kGp3*) of SE(2) / SO(3) / 3-D linear chains -- six rows per state from 11 operands per lane, next to the row ring
  // that still serves measurement factors and velocity priors
  constexpr bool ST12 = ST && B == 12, ST6 = ST && B == 6;
  const FwdArgs<double> &a = u.f;
  static_assert(B == 12 || B == 6, "block sizes with DPP gather blocks");
  static_assert(SV == 0 || B == 12 || SV == 1, "the variants with odd rows are SE(3) variants");
  constexpr int BS = 2 * B * B + B, AS = B * B + B;   // R == 1
  constexpr int NPC = BS / 2, NV = (NPC + 15) / 16;
  typedef double V2 __attribute__((ext_vector_type(2)));
  // (alternating which wave assembles and which eliminates between workgroups -- by bit 0, 1 or 2 of the workgroup index -- so that a
  //  SIMD gets one wave of each kind changes nothing: 0.303-0.307 ms per iteration at 1e5 states for all four assignments)
  const int lane = threadIdx.x & 63, grp = lane >> 4, r = lane & 15;
  int role = threadIdx.x >> 6;
  // (the variants that sit at 256 VGPRs -- a ring of full-width rows next to the records, the general-Qc line form -- keep "wave 0
  //  eliminates": the role bookkeeping costs them 16-20 bytes of scratch, and a scratch reload drains the loads in flight)
  // (block size 6 runs three waves per SIMD, six workgroups per CU: the two-by-two argument above is about two)
  constexpr bool kSwap = B == 12 && !(SV == 3 || (SV == 4 && !DG));
  __shared__ int swap_s;
  int simd_slot = -1;                             // (wave 0: the word it counted itself into)
  if (kSwap && u.simd_cnt != nullptr) {
    if (role == 0) {
      const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xc = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xf;   // HW_ID, XCC_ID
      simd_slot = (int)((((xc * 8 + ((hw >> 13) & 7)) * 2 + ((hw >> 12) & 1)) * 16 + ((hw >> 8) & 0xf)) * 4 + ((hw >> 4) & 3));
      if (lane == 0) swap_s = atomicAdd(u.simd_cnt + simd_slot, 1) > 0 ? 1 : 0;
    }
    __syncthreads();
    role ^= __builtin_amdgcn_readfirstlane(swap_s);
  }
  auto leave = [&]() { if (simd_slot >= 0 && lane == 0) atomicSub(u.simd_cnt + simd_slot, 1); };
  const int c = blockIdx.x * 4 + grp;
  const int nch = (a.n + a.m - 1) / a.m;
  const bool valid = c < nch;
  const int s = valid ? c * a.m : 0;
  const int e = valid ? min(s + a.m, a.n) : 0;
  const int j0 = s + 1;
  const bool rowlane = r < B;
  const int rr = rowlane ? r : 0;
  const bool right_exists = (e < a.n) || (a.last_has_right != 0);
  // tail: the chain's last chunk is padded to full length with decoupled identity blocks (D = I, O = 0, g = 0: their
  // elimination changes nothing and their records are never stored), so that the four chunks of a wave end in the same
  // block step and their separator data is still in registers when the tail starts
  const bool tail = a.tail != 0;
  const int ep = (valid && tail) ? s + a.m : e;
  const bool has_int = valid && j0 < ep;
  const double lambda = a.lambda;
  // The images [D | O | g] the assembly wave hands over are private to this kernel: their rows are padded to BP = B + 1 doubles.
  // With a pitch of B the B lanes of a row access (stride 2 B dwords) collide pairwise in the 64 LDS banks (B = 12: lanes r and
  // r + 8; 32 banks for stores: three ways) -- SQ_LDS_BANK_CONFLICT was 49 % of SQ_LDS_IDX_ACTIVE (round 4); with an odd pitch
  // row accesses and column accesses are both conflict-free inside a 16-lane row.  OUTR keeps the record's own (unpadded,
  // column-major) layout: it leaves as contiguous 16-byte pieces.
  constexpr int BP = B + 1, IS = 2 * B * BP + B + (B & 1);            // image pitch, doubles per image (even)
  __shared__ __attribute__((aligned(16))) double IMG[2 * 4 * IS > 5 * BS + 4 * AS ? 2 * 4 * IS : 5 * BS + 4 * AS];   // two rotating images per chunk (the tail's group reuses the space)
  __shared__ __attribute__((aligned(16))) double OUTR[4 * BS];       // the factor record on its way out
  int ro = grp * IS + rr * BP;    // row r of an image:    IMG[buf * 4 IS + ro + k]          (D: + 0, O: + B BP, g: co + 2 B BP)
  int co = grp * IS + rr;         // column r:             IMG[... + co + k * BP]
  int po = grp * BS + 2 * r;      // 16-byte piece q * 16 + r of OUTR
  int oc = grp * BS + rr;         // column r of the factor record in OUTR: OUTR[oc + k * B]
  int tr = grp * BS + rr * BP;    // row r of the (padded) transpose scratch inside OUTR's V | U area
  int tc = grp * BS + rr;         // ... its column r: OUTR[tc + k * BP]
  asm volatile("" : "+v"(ro), "+v"(co), "+v"(po), "+v"(oc), "+v"(tr), "+v"(tc));
  const int steps = __builtin_amdgcn_readfirstlane(max(ep - j0, 0));   // lane 0: the wave's first (never shorter) chunk
  GPS_TR(0);
#ifdef GPS_TRACE_FUSED
  if (u.trace && lane == 0) {
    u.trace[((size_t)blockIdx.x * 2 + role) * 64 + 61] = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_ID
    u.trace[((size_t)blockIdx.x * 2 + role) * 64 + 62] = __builtin_amdgcn_s_getreg((31 << 11) | 20);    // XCC_ID
  }
#endif

  if (role == 1) {
    // ================================================================ ASM: images 0 .. steps + 1
    // Everything that has a memory latency is requested one state ahead: the row pointers of state t + 2 and the first
    // PF rows (full-width and compact) of state t + 1 are in flight while state t is accumulated.
    // ring depths (rows in flight per table).  Whole-state rings (12 full-width rows: one GP prior) were measured SLOWER
    // (0.197 vs 0.182 ms): with all arithmetic of both waves ablated the kernel still takes 0.158 ms -- 313 MB of row reads
    // + 248 MB of factor writes at the mixed read / write rate this part sustains -- so deeper prefetch only costs registers.
    constexpr int PF = ST6 ? 3 : (ORING ? (DG ? 6 : 4) : 6), PC = ST12 ? (SV == 2 ? 4 : ((ORING || IROW) ? 2 : 1)) : (ST6 ? 3 : 6), Dh = B / 2;
    constexpr int PFI = 12;                               // interpolated rows in flight: one register each (four GPS factors of an interval)   // (ST6: three waves per SIMD need <= 168 VGPRs)   // (ST: the records take the registers of the compact ring: pose priors are what is left in it)
    const int rc = r < Dh ? r : 0;
    const int ptr_max = a.n + 1;                         // rowptr / crowptr have n + 2 entries
    // R^T R of the state's rows (and its share of the gradient): what opens the NEXT state's D -- kept where it is summed, the next
    // state takes it over when it starts (round 4: a copy out at the end of a state and a copy in at the start of the next were
    // 24 moves per state); dgpend: what write_img adds to the diagonal of the image (LM damping, identity of a padding block)
    double RRacc[B], grr = 0.0, dgpend = 0.0;
#pragma unroll
    for (int k = 0; k < B; k++) RRacc[k] = 0.0;
    double Dacc[B], Oacc[B], gacc;
    constexpr bool FRING = !ST12 || ORING;            // a ring of full-width rows (ORING: 4 deep -- 6 in the diagonal-Qc form -- + 2 compact rows is what 256 VGPRs hold next to the records)
    double fL[FRING ? PF : 1], fR[FRING ? PF : 1], fE[FRING ? PF : 1], cL[PC], cR[PC], cE[PC];   // the two operand rings
    double fI[IROW ? PFI : 1];                           // ... and the ring of interpolated rows: element (lane & 15) of each line
    // IROW (round 6): the compact rows (a between factor's six, a pose prior's) as ONE register per row as well -- lane c < 12 holds
    // element c of [L (6) | R (6)], lanes 12..15 the whitened error -- so that a whole state's rows are in flight where the three
    // registers per row of cL / cR / cE allowed two: their latency was exposed three times per block step (2.2 of its 7.1 us)
    constexpr int PCI = 6;
    double cV[IROW ? PCI : 1];
    const int *fptr = IROW ? u.irowptr : u.rowptr;       // the full-width table this variant walks
    int rp = 0, nf = 0, cp = 0, nc = 0;                  // rows of the state the rings belong to
    int rpn = fptr[min(s + 1, ptr_max)], cpn = u.crowptr[min(s + 1, ptr_max)];      // pointers one state ahead
    int rpnn = fptr[min(s + 2, ptr_max)], cpnn = u.crowptr[min(s + 2, ptr_max)];    // ... and two
    // structured GP prior of the state (u.gps, layout kGps*): lane c < 12 of the chunk's DPP row builds COLUMN c of the whitened
    // [L | R] from the record's blocks -- pose columns for c < 6, velocity columns for c >= 6 (see the record's description):
    //   column r6 = c mod 6 of X = Jinv and of J as six-vectors [top; bottom] (the translation columns have a zero top and
    //   the diagonal block below it), F times both (F's blocks live one entry per lane: element 3 i + j in lane 3 i + j),
    //   then  L = [U (aL J_c + b F J_c); U (c F J_c - dR J_c)],  R = [U (aR X_c + b F X_c); U (c F X_c + dR X_c)]
    // with per-lane coefficients fetched from the record (pose lanes: aL = aR = sa, b = sb, c = sc, dR = 0; velocity lanes:
    // J_c = the unit vector, aL = k2, aR = sb, b = c = 0, dR = sc -- their zeros are the record's zero slot).
    constexpr bool st_on = ST;
    constexpr int NRAW = ST12 ? 21 : (ST6 ? 11 : 1);
    double Ur[(ST12 && !DG) ? 3 : 1];
    if constexpr (ST12 && !DG) {
#pragma unroll
      for (int k = 0; k < 3; k++) Ur[k] = u.Ud[min(16 * k + r, 35)];       // U, row-major: entry e in lane e & 15 of Ur[e >> 4]
    }
    double udv = 0.0;                                                        // DG: the diagonal, entry k in lane k of every row
    if constexpr (DG) udv = u.Ud[7 * min(r, 5)];
    // where this lane's operands sit in a record (loop-invariant; the stride-3 walks down a column are immediate offsets)
    int oX1 = 0, oX2 = 0, oJ1 = 0, oJ2 = 0, oF = 0, oE = 0, oaL = 0, oaR = 0, ob = 0, oc = 0, od = 0;
    if constexpr (ST12) {
      const int r6 = r < Dh ? r : (r < B ? r - Dh : 0);
      const bool velc = r >= Dh && r < B, hi3 = r6 >= 3;
      const int j3 = hi3 ? r6 - 3 : r6;
      oX1 = kGpsXA + j3; oX2 = (hi3 ? kGpsXA : kGpsXC) + j3;      // top three of X's column (masked for the translation columns), bottom three
      oJ1 = kGpsJA + j3; oJ2 = (hi3 ? kGpsJA : kGpsJC) + j3;
      oF = min(r, 8); oE = kGpsE + min(r, 11);
      oaL = velc ? kGpsS + 0 : kGpsS + 3;    // aL: k2 | sa
      oaR = velc ? kGpsS + 1 : kGpsS + 3;    // aR: sb | sa
      ob = velc ? kGpsZ : kGpsS + 1;         // b:  0  | sb
      oc = velc ? kGpsZ : kGpsS + 2;         // c:  0  | sc
      od = velc ? kGpsS + 2 : kGpsZ;         // dR: sc | 0
    }
    double raw[NRAW];
    int gp = -1;
    // BetweenFactor<Pose3> record of the state (u.brec, kBtw*): lane c < 6 builds column c of [H1 | H2] from the block-triangular
    // halves exactly as above (the same column walk: oX1 / oX2 minus their bases), lanes 6..11 read the all-zero record
    constexpr int NBR = ST12 ? 14 : 1;
    double braw[NBR];
    // (not in the variant with odd full-width rows: its registers are spoken for -- the host hands it compact rows)
    const bool btw_on = ST12 && !ODD && u.brec != nullptr;
    int bq = -1, bqn = btw_on ? u.btwidx[min(s + 1, ptr_max)] : -1, bqnn = btw_on ? u.btwidx[min(s + 2, ptr_max)] : -1;
#pragma unroll
    for (int k = 0; k < NBR; k++) braw[k] = 0.0;
    auto ldbtw = [&]() {                      // operands of the between factor whose left state the rings point at (bq)
      if constexpr (ST12) {
        if (!btw_on) return;                  // (no records on this launch: u.brec is null)
        const double *rec = u.brec + (size_t)((bq >= 0 && r < Dh) ? bq : u.btw_count) * kBtwLen;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          braw[k] = rec[kBtwRA - kGpsXA + oX1 + 3 * k]; braw[3 + k] = rec[kBtwRA - kGpsXA + oX2 + 3 * k];
          braw[6 + k] = rec[kBtwLA - kGpsXA + oX1 + 3 * k]; braw[9 + k] = rec[kBtwLA - kGpsXA + oX2 + 3 * k];
        }
        braw[12] = rec[kBtwW + min(r, Dh - 1)];
        braw[13] = rec[kBtwE + min(r, Dh - 1)];
      }
    };
    int gpn = st_on ? u.gpidx[min(s + 1, ptr_max)] : -1, gpnn = st_on ? u.gpidx[min(s + 2, ptr_max)] : -1;
    // operands of the GP prior whose left state is s + kimg (record g; no such factor: the all-zero record behind the last one)
    auto ldraw = [&](int kimg, int g) {
      if constexpr (ST6) {
        // d = 3 record (kGp3*): lane c < 6 holds column c of the six rows [A1 | kLt U | A3 | kRt U; 0 | kLb U | 0 | kRb U] -- a pose
        // lane (c < 3) its column of A1 / A3, a velocity lane column c - 3 of U and the record's four coefficients; lane q < 6 also
        // fetches whitened error q (it travels by row_newbcast)
        const bool live = valid && (s + kimg) < e && g >= 0;
        const double *rec = u.gps + (size_t)(live ? g : u.gp_count) * kGp3Len;
        const bool pc = r < 3;
        const int c3 = pc ? r : (r < 6 ? r - 3 : 0);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          raw[k] = pc ? rec[kGp3A1 + 3 * k + c3] : u.Ud[3 * k + c3];
          raw[3 + k] = pc ? rec[kGp3A3 + 3 * k + c3] : u.Ud[3 * k + c3];
        }
        // (the zero record makes the velocity lanes' coefficients zero: a state without a GP prior contributes nothing)
        raw[6] = rec[kGp3S + 0]; raw[7] = rec[kGp3S + 1]; raw[8] = rec[kGp3S + 2]; raw[9] = rec[kGp3S + 3];
        raw[10] = rec[kGp3E + min(r, 5)];
      }
      if constexpr (ST12) {
        const bool live = valid && (s + kimg) < e && g >= 0;
        const double *rec = u.gps + (size_t)(live ? g : u.gp_count) * kGpsLen;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          raw[k] = rec[oX1 + 3 * k]; raw[3 + k] = rec[oX2 + 3 * k];
          raw[6 + k] = rec[oJ1 + 3 * k]; raw[9 + k] = rec[oJ2 + 3 * k];
        }
        raw[12] = rec[kGpsFA + oF]; raw[13] = rec[kGpsFC + oF]; raw[14] = rec[kGpsFD + oF];
        raw[15] = rec[oE];
        raw[16] = rec[oaL]; raw[17] = rec[oaR]; raw[18] = rec[ob]; raw[19] = rec[oc]; raw[20] = rec[od];
      }
    };
    double Lcol[ST12 ? B : 1], Rcol[ST12 ? B : 1], newl = 0.0;
    auto reconstruct = [&]() {
      if constexpr (ST12) {
        double X6[6], J6[6], P3[6], P1[6];
        // the lane's role, recomputed per state from an opaque copy of its index: as loop invariants the masks and the unit
        // vector would occupy two dozen registers for the whole kernel (the wave spilled with them)
        int rq = r;
        asm volatile("" : "+v"(rq));
        const bool tcol = (rq >= 3 && rq < 6) || (rq >= 9), vcol = rq >= 6;   // translation column; velocity column
#pragma unroll
        for (int k = 0; k < 3; k++) {
          X6[k] = tcol ? 0.0 : raw[k]; X6[3 + k] = raw[3 + k];
          J6[k] = vcol ? ((rq == 6 + k) ? 1.0 : 0.0) : (tcol ? 0.0 : raw[6 + k]);
          J6[3 + k] = vcol ? ((rq == 9 + k) ? 1.0 : 0.0) : raw[9 + k];
        }
#pragma unroll
        for (int k = 0; k < 6; k++) { P3[k] = 0.0; P1[k] = 0.0; }
        const double *fa = &raw[12], *fc = &raw[13], *fd = &raw[14];
        static_for<0, 3>([&](auto jj) {            // F [top; bottom] = [FA top; FC top + FD bottom]
          constexpr int j = decltype(jj)::value;
          fmac_mat<3, j, 3>(P3, fa, X6[j]);
          fmac_mat<3, j, 3>(P3 + 3, fc, X6[j]);
          fmac_mat<3, j, 3>(P3 + 3, fd, X6[3 + j]);
          fmac_mat<3, j, 3>(P1, fa, J6[j]);
          fmac_mat<3, j, 3>(P1 + 3, fc, J6[j]);
          fmac_mat<3, j, 3>(P1 + 3, fd, J6[3 + j]);
        });
        const double aL = raw[16], aR = raw[17], bb = raw[18], cc = raw[19], dR = raw[20], ndR = -dR;
        double Z[4][6];
#pragma unroll
        for (int k = 0; k < 6; k++) {
          Z[0][k] = fma(aL, J6[k], bb * P1[k]);      // top rows of L
          Z[1][k] = fma(cc, P1[k], ndR * J6[k]);     // bottom rows of L
          Z[2][k] = fma(aR, X6[k], bb * P3[k]);      // top rows of R
          Z[3][k] = fma(cc, P3[k], dR * X6[k]);      // bottom rows of R
        }
        if constexpr (DG) {
          static_for<0, 6>([&](auto kk) {            // U Z, U diagonal
            constexpr int k = decltype(kk)::value;
            const double uk = row_bcast<k>(udv);
            Lcol[k] = uk * Z[0][k]; Lcol[6 + k] = uk * Z[1][k];
            Rcol[k] = uk * Z[2][k]; Rcol[6 + k] = uk * Z[3][k];
            // (formed here: sunk into the row loop they would keep Z and the record's operands alive across it -- the wave spilled)
            asm volatile("" : "+v"(Lcol[k]), "+v"(Lcol[6 + k]), "+v"(Rcol[k]), "+v"(Rcol[6 + k]));
          });
        } else {
#pragma unroll
          for (int k = 0; k < B; k++) { Lcol[k] = 0.0; Rcol[k] = 0.0; }
          static_for<0, 6>([&](auto kk) {            // U Z, U upper triangular: out[i] += U[i][k] Z[k], i <= k
            constexpr int k = decltype(kk)::value;
            fmac_mat<k + 1, k, 6>(Lcol, Ur, Z[0][k]);
            fmac_mat<k + 1, k, 6>(Lcol + 6, Ur, Z[1][k]);
            fmac_mat<k + 1, k, 6>(Rcol, Ur, Z[2][k]);
            fmac_mat<k + 1, k, 6>(Rcol + 6, Ur, Z[3][k]);
          });
        }
        newl = -raw[15];                             // minus the whitened error of row (lane)
      }
    };
    auto ldf = [&](int i, double &Lv, double &Rv, double &ev) {
      const int rho = rp + min(i, max(nf - 1, 0));
      const TR *row = u.rowLR + (size_t)rho * 2 * B;
      Lv = (double)row[rr]; Rv = (double)row[B + rr]; ev = (double)u.rowE[rho];
    };
    auto ldfi = [&](int i, double &v) {      // element (lane & 15) of interpolated row i of the state the rings point at
      const int rho = rp + min(i, max(nf - 1, 0));
      v = u.rowI[(size_t)rho * kIRowLen + r];
    };
    // point the ring of interpolated rows at state s + kimg and request its first PFI lines.  assemble() does this for the NEXT
    // state as soon as the current state's lines are consumed (they then travel under the GP prior's, the between factor's and the
    // pose prior's rows: ~800 instructions); open_state() only for the very first state.
    bool iopened = false;
    auto open_irows = [&](int kimg, int p0, int p1) {
      const bool live = valid && (s + kimg) < e;
      rp = live ? p0 : 0; nf = live ? p1 - p0 : 0;
#pragma unroll
      for (int q = 0; q < PFI; q++) ldfi(q, fI[q]);
      iopened = true;
    };
    auto ldc = [&](int i, double &Lv, double &Rv, double &ev) {
      const int rho = cp + min(i, max(nc - 1, 0));
      const TR *row = u.rowC + (size_t)rho * B;
      Lv = (double)row[rc]; Rv = (double)row[Dh + rc]; ev = (double)u.rowCE[rho];
    };
    auto ldcv = [&](int i, double &v) {      // element (lane & 15) of compact row i of the state the rings point at: [L | R | e e e e]
      const int rho = cp + min(i, max(nc - 1, 0));
      const TR *p = (r < B) ? u.rowC + (size_t)rho * B + r : u.rowCE + rho;
      v = (double)*p;
    };
    // point the rings at state s + kimg (row range known from the pointers loaded earlier) and start their first loads
    auto open_state = [&](int kimg, int p0, int p1, int q0, int q1, int g, int bqv) {
      const bool live = valid && (s + kimg) < e;
      gp = (live && st_on) ? g : -1;
      bq = (live && btw_on) ? bqv : -1;
      if (gp >= 0 && !IROW) p0 += B;                     // its 12 rows lead the state's range in the row table: not used (the table of interpolated rows never held them)
      if (bq >= 0) q1 -= Dh;                             // ... and its between factor's six rows end its range in the compact table
      if constexpr (!IROW) { rp = (live && (!ST12 || ODD)) ? p0 : 0; nf = (live && (!ST12 || ODD)) ? p1 - p0 : 0; }   // (ODD: the few other full-width rows)
      cp = live ? q0 : 0; nc = live ? q1 - q0 : 0;
      if constexpr (FRING) {
#pragma unroll
        for (int q = 0; q < PF; q++) ldf(q, fL[q], fR[q], fE[q]);
      }
      if constexpr (IROW) {
        if (!iopened) open_irows(kimg, p0, p1);          // (the first state only: every other one was opened early, by assemble)
        iopened = false;
      } else {       // (IROW: the compact ring of a state is requested behind that state's interpolated rows, whose loop needs the registers)
#pragma unroll
        for (int q = 0; q < PC; q++) ldc(q, cL[q], cR[q], cE[q]);
      }
    };
    auto assemble = [&](int kimg) {
      const bool live = valid && (s + kimg) < e;
      GPS_TRA(40);
      int nfm = nf, ncm = nc;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { nfm = max(nfm, __shfl_xor(nfm, o, 64)); ncm = max(ncm, __shfl_xor(ncm, o, 64)); }
      nfm = __builtin_amdgcn_readfirstlane(nfm);
      ncm = __builtin_amdgcn_readfirstlane(ncm);
#pragma unroll
      for (int k = 0; k < B; k++) { Dacc[k] = RRacc[k]; Oacc[k] = 0.0; RRacc[k] = 0.0; }
      gacc = grr;
      grr = 0.0;
      if constexpr (IROW) {
        // The interpolated measurement rows of the state FIRST, while the record's operands are still whole (the columns of the
        // GP prior are formed after this loop, into the registers it frees).  Row = [Lp | mu | e, p11, p12, l12], one element per
        // lane:  L = [Lp | l12 mu],  R = [mu (p11 X + p12 F X) | p12 mu X] = cA (mu . Xc) + cB (mu . Pc)  with this lane's column
        // Xc of X (velocity lanes: column c - 6) and Pc = F Xc, (cA, cB) = (p11, p12) on pose lanes, (p12, 0) on velocity lanes.
        int rq = r;
        asm volatile("" : "+v"(rq));
        const bool tcol = (rq >= 3 && rq < 6) || (rq >= 9), posel = rq < Dh, vell = rq >= Dh && rq < B;
        double Xc[6], Pc[6];
#pragma unroll
        for (int k = 0; k < 3; k++) { Xc[k] = tcol ? 0.0 : raw[k]; Xc[3 + k] = raw[3 + k]; }
#pragma unroll
        for (int k = 0; k < 6; k++) Pc[k] = 0.0;
        static_for<0, 3>([&](auto jj) {                  // F [top; bottom] = [FA top; FC top + FD bottom]
          constexpr int j = decltype(jj)::value;
          fmac_mat<3, j, 3>(Pc, &raw[12], Xc[j]);
          fmac_mat<3, j, 3>(Pc + 3, &raw[13], Xc[j]);
          fmac_mat<3, j, 3>(Pc + 3, &raw[14], Xc[3 + j]);
        });
        for (int i0 = 0; i0 < nfm; i0 += PFI) {
          if (i0 > 0) {                                  // more than PFI lines on one state (rare): the ring is refilled in place
#pragma unroll
            for (int q = 0; q < PFI; q++) ldfi(i0 + q, fI[q]);
          }
#pragma unroll
          for (int q = 0; q < PFI; q++) {
            const int i = i0 + q;
            const double V = (i < nf) ? fI[q] : 0.0;
            double sc[4];
            row_bcast4_at<kIRowE>(V, sc);                // whitened error, p11, p12, l12
            const double Lv = posel ? V : (vell ? sc[3] * V : 0.0);
            double sX = 0.0, sP = 0.0;
            fmac_dot6x2_at<kIRowMu>(sX, sP, V, Xc, Pc);  // mu . Xc, mu . Pc
            const double cA = posel ? sc[1] : sc[2], cB = posel ? sc[2] : 0.0;
            const double Rv = rowlane ? fma(cA, sX, cB * sP) : 0.0;
            fmac_gather<B>(Dacc, Lv, Lv);
            fmac_gather<B>(Oacc, Lv, Rv);
            fmac_gather<B>(RRacc, Rv, Rv);
            gacc = fma(-Lv, sc[0], gacc);
            grr = fma(-Rv, sc[0], grr);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        open_irows(kimg + 1, rpn, rpnn);                 // the next state's lines: in flight under the rest of this state
#pragma unroll
        for (int q = 0; q < PCI; q++) ldcv(q, cV[q]);    // this state's compact rows: wanted behind the GP prior's twelve
      }
      if constexpr (ST6) {                               // the d = 3 record: six rows from the lane's column of [A1 | U | A3 | U]
        const bool pc = r < 3;
        const double mLt = pc ? 1.0 : raw[6], mRt = pc ? 1.0 : raw[7], mLb = pc ? 0.0 : raw[8], mRb = pc ? 0.0 : raw[9];
        const double ne3 = -raw[10];
        static_for<0, 6>([&](auto ii) {
          constexpr int i = decltype(ii)::value;
          const double Lv = (i < 3 ? mLt : mLb) * raw[i % 3], Rv = (i < 3 ? mRt : mRb) * raw[3 + i % 3];
          fmac_gather<B>(Dacc, Lv, Lv);
          fmac_gather<B>(Oacc, Lv, Rv);
          fmac_gather<B>(RRacc, Rv, Rv);
          fmac_bcast2<i>(gacc, grr, ne3, Lv, Rv);
          __builtin_amdgcn_sched_barrier(0);
        });
        ldraw(kimg + 1, gpn);                            // (the operands are consumed: the next state's record into their registers)
      }
      if constexpr (ST12) {                              // the structured GP prior: its 12 rows from the columns built above
        GPS_TRA(41);
        reconstruct();
        GPS_TRA(42);
        static_for<0, B>([&](auto qq) {
          constexpr int q = decltype(qq)::value;
          // the next state's record is requested once most of this state's columns are consumed (their registers take it)
          if constexpr (q == 8) ldraw(kimg + 1, gpn);
          if constexpr (q == 5) ldbtw();                 // this state's between record: wanted right behind these twelve rows
          const double Lv = Lcol[q], Rv = Rcol[q];
          // (round 6: unguarded multiply-adds -- what they read through DPP, the row's entries Lcol[q] / Rcol[q] and the whitened
          //  error, was written by reconstruct() before this loop began; one guard opens the loop)
          if constexpr (q == 0) dpp_guard();
          if constexpr (DG) {
            // row q of L: the pose columns and velocity column 6 + q mod 6.  X, J and F are block lower triangular ([[A, 0], [C, D]]),
            // so the rotation rows (q mod 6 < 3) of the whitened [L | R] are zero in every translation column (3..5, and 9..11 of R)
            constexpr int vq = Dh + q % Dh;
            if constexpr (q % Dh < 3) {
              fmac_gather_nn<3>(Dacc, Lv, Lv); fmac_bcast1_nn<vq>(Dacc[vq], Lv, Lv);
              fmac_gather_nn<3>(Oacc, Lv, Rv); fmac_bcast1_nn<vq>(Oacc[vq], Lv, Rv);
              fmac_gather_nn<3>(RRacc, Rv, Rv); fmac_gather_nn<3, Dh>(RRacc + Dh, Rv, Rv);
            } else {
              fmac_gather_nn<Dh>(Dacc, Lv, Lv); fmac_bcast1_nn<vq>(Dacc[vq], Lv, Lv);
              fmac_gather_nn<Dh>(Oacc, Lv, Rv); fmac_bcast1_nn<vq>(Oacc[vq], Lv, Rv);
              fmac_gather_nn<B>(RRacc, Rv, Rv);
            }
          } else {
            fmac_gather_nn<B>(Dacc, Lv, Lv);
            fmac_gather_nn<B>(Oacc, Lv, Rv);
            fmac_gather_nn<B>(RRacc, Rv, Rv);
          }
          fmac_bcast1_nn<q>(gacc, newl, Lv);             // g -= e[q] L[q][r]
          fmac_bcast1_nn<q>(grr, newl, Rv);              // carry_g -= e[q] R[q][r]
          __builtin_amdgcn_sched_barrier(0);
        });
      }
      GPS_TRA(43);
      if (kimg >= 3) fused_step_prio<B>(2 * (kimg - 3) + 1);   // (image t + 3 is assembled under block step t: its middle)
      if constexpr (ST12) {                              // the state's BetweenFactor<Pose3> record: six compact rows from its columns
        if (btw_on) {
          int rq = r;
          asm volatile("" : "+v"(rq));
          const bool tcol = rq >= 3;                     // translation columns: zero top, the diagonal block below
          double Lc6[6], Rc6[6];
#pragma unroll
          for (int k = 0; k < 3; k++) {
            Rc6[k] = tcol ? 0.0 : braw[k]; Rc6[3 + k] = braw[3 + k];
            Lc6[k] = tcol ? 0.0 : braw[6 + k]; Lc6[3 + k] = braw[9 + k];
          }
          const double nbe = -braw[13];
          static_for<0, Dh>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            const double wi = row_bcast<i>(braw[12]);     // 1 / sigma of row i
            const double Lv = wi * Lc6[i], Rv = wi * Rc6[i];
            dpp_guard();                                 // (Lv, Rv are one instruction old; everything else in the row is not)
            if constexpr (i < 3) {                       // rotation rows of [[A, 0], [C, A]]: zero in the translation columns
              fmac_gather_nn<3>(Dacc, Lv, Lv);
              fmac_gather_nn<3>(Oacc, Lv, Rv);
              fmac_gather_nn<3>(RRacc, Rv, Rv);
            } else {
              fmac_gather_nn<Dh>(Dacc, Lv, Lv);
              fmac_gather_nn<Dh>(Oacc, Lv, Rv);
              fmac_gather_nn<Dh>(RRacc, Rv, Rv);
            }
            fmac_bcast1_nn<i>(gacc, nbe, Lv);
            fmac_bcast1_nn<i>(grr, nbe, Rv);
            __builtin_amdgcn_sched_barrier(0);
          });
        }
      }
      GPS_TRA(44);
      if constexpr (SV == 2) {
        // the odd full-width row of a structured chain (host-checked to be few): fetched where it is used, no ring --
        // only the block step of a state that has one waits for it
        for (int i = 0; i < nfm; i++) {
          double Lv, Rv, ev;
          ldf(i, Lv, Rv, ev);
          const bool ok = i < nf;
          Lv = ok ? Lv : 0.0; Rv = ok ? Rv : 0.0; ev = ok ? ev : 0.0;
          fmac_gather<B>(Dacc, Lv, Lv);
          fmac_gather<B>(Oacc, Lv, Rv);
          fmac_gather<B>(RRacc, Rv, Rv);
          gacc = fma(-Lv, ev, gacc);
          grr = fma(-Rv, ev, grr);
        }
      }
      if constexpr (FRING)
      for (int i0 = 0; i0 < nfm; i0 += PF) {             // full-width rows
#pragma unroll
        for (int q = 0; q < PF; q++) {
          const int i = i0 + q;
          const bool ok = i < nf;
          const double Lv = ok ? fL[q] : 0.0, Rv = ok ? fR[q] : 0.0, ev = ok ? fE[q] : 0.0;
          fmac_gather<B>(Dacc, Lv, Lv);     // D[r][k] += L[k] L[r]: the row's element of lane k fused into the multiply-add
          fmac_gather<B>(Oacc, Lv, Rv);     // O[r][k] += L[k] R[r]
          fmac_gather<B>(RRacc, Rv, Rv);    // carry[r][k] += R[k] R[r]
          gacc = fma(-Lv, ev, gacc);
          grr = fma(-Rv, ev, grr);
          ldf(i + PF, fL[q], fR[q], fE[q]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if constexpr (IROW) {
        for (int i0 = 0; i0 < ncm; i0 += PCI) {          // compact rows, one register each (see cV)
          if (i0 > 0) {                                  // more than PCI on one state (a pose prior next to a between factor): refilled in place
#pragma unroll
            for (int q = 0; q < PCI; q++) ldcv(i0 + q, cV[q]);
          }
#pragma unroll
          for (int q = 0; q < PCI; q++) {
            const int i = i0 + q;
            const double V = (i < nc) ? cV[q] : 0.0;
            // this lane's R entry sits six lanes up (row_shl:6, zero where the source lane falls off the row)
            const int rlo = __builtin_amdgcn_update_dpp(0, __double2loint(V), 0x106, 0xf, 0xf, true);
            const int rhi = __builtin_amdgcn_update_dpp(0, __double2hiint(V), 0x106, 0xf, 0xf, true);
            const bool pl = r < Dh;
            const double Lv = pl ? V : 0.0, Rv = pl ? __hiloint2double(rhi, rlo) : 0.0;
            const double ev = row_bcast<B>(V);
            fmac_gather<Dh>(Dacc, V, Lv);                 // D[r][k] += L[k] L[r]   (lane k < 6 of V holds L[k])
            fmac_gather<Dh>(Oacc, V, Rv);                 // O[r][k] += L[k] R[r]
            fmac_gather_nn<Dh, Dh>(RRacc, V, Rv);         // carry[r][k] += R[k] R[r]   (lane 6 + k holds R[k]; V was guarded above)
            gacc = fma(-Lv, ev, gacc);
            grr = fma(-Rv, ev, grr);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else
      for (int i0 = 0; i0 < ncm; i0 += PC) {             // compact rows (velocity-free): six columns each side
#pragma unroll
        for (int q = 0; q < PC; q++) {
          const int i = i0 + q;
          const bool ok = (i < nc) && (r < Dh);
          const double Lv = ok ? cL[q] : 0.0, Rv = ok ? cR[q] : 0.0, ev = (i < nc) ? cE[q] : 0.0;
          fmac_gather<Dh>(Dacc, Lv, Lv);
          fmac_gather<Dh>(Oacc, Lv, Rv);
          fmac_gather<Dh>(RRacc, Rv, Rv);
          gacc = fma(-Lv, ev, gacc);
          grr = fma(-Rv, ev, grr);
          ldc(i + PC, cL[q], cR[q], cE[q]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      GPS_TRA(45);
      {   // Levenberg-Marquardt damping on the diagonal of a real state's D; the padding blocks behind the chain's last state
          // (tail) are identities
        // (added by write_img to the image's diagonal entry, one LDS read-modify-write of the lane's own row: as a select over the
        //  twelve column registers it was 24 instructions per state, for a zero in every Gauss-Newton iteration)
        const bool pad = valid && (s + kimg) >= e && (s + kimg) < ep;
        dgpend = live ? lambda : (pad ? 1.0 : 0.0);
      }
      // the next state: its row range is known, open its rings; fetch the pointers of the state after it
      open_state(kimg + 1, rpn, rpnn, cpn, cpnn, gpn, bqn);
      rpn = rpnn; cpn = cpnn; gpn = gpnn; bqn = bqnn;
      if (btw_on) bqnn = u.btwidx[min(s + kimg + 3, ptr_max)];
      rpnn = fptr[min(s + kimg + 3, ptr_max)];
      cpnn = u.crowptr[min(s + kimg + 3, ptr_max)];
      if (st_on) gpnn = u.gpidx[min(s + kimg + 3, ptr_max)];
      GPS_TRA(46);
    };
    auto write_img = [&](int buf, int kimg) {
      if (rowlane) {
        double *img = IMG + buf * 4 * IS;
#pragma unroll
        for (int k = 0; k < B; k++) { img[ro + k] = Dacc[k]; img[ro + B * BP + k] = Oacc[k]; }
        if (dgpend != 0.0) { const double t = img[ro + rr]; img[ro + rr] = t + dgpend; }   // D[r][r] += lambda (or the padding block's 1)
        img[co + 2 * B * BP] = gacc;
        if (u.gsave && valid) {          // (LM) the gradient: a state's own record, and what the chunk's last rows owe the next separator
          const int jg = s + kimg;
          if (jg < e) u.gsave[(size_t)jg * B + r] = gacc;
          else if (jg == e && e < a.n) u.gsave2[(size_t)e * B + r] = gacc;
        }
      }
    };
    {
      const int g0 = st_on ? u.gpidx[min(s, ptr_max)] : -1;
      ldraw(0, g0);
      open_state(0, fptr[min(s, ptr_max)], rpn, u.crowptr[min(s, ptr_max)], cpn, g0, btw_on ? u.btwidx[min(s, ptr_max)] : -1);
    }
    assemble(0); write_img(0, 0);
    assemble(1); write_img(1, 1);
    GPS_TR(1);
    lds_barrier();                       // P: images 0 and 1 are there
    lds_barrier();                       // Q: ELIM has taken what it needs from image 0
    GPS_TR(2);
    // (round 3: image 2 is assembled AFTER Q, under the elimination of the first block -- ELIM only needs it at the barrier
    //  of step 0.  Before, ELIM sat at Q through this assembly: one block step of every chunk, 3 % of the kernel)
    assemble(2);
    write_img(0, 2);
    for (int t = 0; t < steps; t++) {
      fused_step_prio<B>(2 * t);
      GPS_TR(3 + min(t, 50));
      lds_barrier();                     // step t: image t + 2 is there; image t + 1 is dead from here on
      if (t + 1 < steps) { assemble(t + 3); write_img((t + 1) & 1, t + 3); }
    }
    GPS_TR(60);
    leave();
    return;
  }

  // ================================================================== ELIM (k_chunk_forward_rows on LDS images)
  double Dr[B], Or[B], Fr[B], Gr[B], Ar[B];
  double gr, as_;
  lds_barrier();                         // P
  GPS_TR(1);
#pragma unroll
  for (int k = 0; k < B; k++) {
    Ar[k] = IMG[ro + k];                           // image 0: the separator
    Fr[k] = IMG[ro + B * BP + k];
    Gr[k] = IMG[co + B * BP + k * BP];
    Dr[k] = IMG[4 * IS + ro + k];                  // image 1: the first interior state (or the virtual end record)
    Or[k] = IMG[4 * IS + co + B * BP + k * BP];
  }
  as_ = IMG[co + 2 * B * BP];
  gr = IMG[4 * IS + co + 2 * B * BP];
  lds_barrier();                         // Q
  GPS_TR(2);
  if (valid && !has_int && rowlane) {    // chunk without interior: the separator keeps its coupling, its rows' R^T R is owed
    double *ub = a.up_blk + (size_t)c * BS;
#pragma unroll
    for (int k = 0; k < B; k++) {
      ub[r * B + k] = Ar[k];
      ub[B * B + r * B + k] = right_exists ? Fr[k] : 0.0;
    }
    ub[2 * B * B + r] = as_;
    if (right_exists) {
      double *ua = a.up_add + (size_t)(c + 1) * AS;
#pragma unroll
      for (int k = 0; k < B; k++) ua[r * B + k] = Dr[k];
      ua[B * B + r] = gr;
    }
  }
  for (int t = 0; t < steps; t++) {
    fused_step_prio<B>(2 * t);
    const int j = j0 + t;
    const bool live = j < e, lastb = (j == e - 1);
    const double *cur = IMG + ((t + 1) & 1) * 4 * IS, *nxt = IMG + (t & 1) * 4 * IS;   // images t + 1 and t + 2
    // Round 6: the elimination wave is the wave a block step waits for (scripts/trace_fused.py: the assembly wave sits at the
    // barrier 0.65-1.0 us of a 4.6-5.6 us step), and alone on a SIMD it issued one instruction per 8 cycles -- it waited for its own
    // dependent chains.  Same arithmetic, same operands, same order of every sum (bit-identical), rearranged so that no latency is
    // exposed to this wave:
    //  * the reciprocal of pivot k + 1 (broadcast, v_rcp_f64, two Newton steps, the multiplier: nine dependent instructions) is
    //    started as soon as column k + 1 of D~ has taken pivot k's update, and its steps are dealt between the row operations on
    //    O, F and g that follow;
    //  * the columns right of the pivot are updated exactly (66 instead of 84 multiply-adds per block: no blocks of four);
    //  * row r of O_j is requested before the elimination instead of behind it; the diagonal block of the next image and the
    //    pieces of the outgoing factor record are requested together behind the barrier and consumed behind the 288 products with
    //    V_j (F_{j+1}, D_sep), the transposed G_{j+1} and the next O^T behind the 144 products with U_j;
    //  * the multiply-adds carry no s_nop (dpp.hpp: the DPP source of every one of them was written a pivot step earlier).
    GPS_TRE(48);
    double Ol[B];
#pragma unroll
    for (int k = 0; k < B; k++) Ol[k] = cur[ro + B * BP + k];         // row r of O_j (image t + 1: published a step ago)
    double invs = 1.0;
    double inv = fast_rcp(row_bcast<0>(Dr[0]));
    static_for<0, B>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      const bool isk = (r == k);
      invs = isk ? inv : invs;
      const double nmp = isk ? 0.0 : -(Dr[k] * inv);
      // row r -= (D~[r][k] / pivot) * row k, the pivot row fused into the multiply-add
      double pn = 1.0, rn = 1.0;
      if constexpr (k + 1 < B) {
        fmac_self1_nn<k>(Dr[k + 1], nmp);                // the next pivot's column first ...
        pn = row_bcast<k + 1>(Dr[k + 1]);                // (guarded: Dr[k + 1] was written by the instruction before)
        rn = __builtin_amdgcn_rcp(pn);                   // ... and its reciprocal under way beneath what follows
        fmac_self_range_nn<k, (k + 2 < B ? k + 2 : B), B>(Dr, nmp);
      }
      __builtin_amdgcn_sched_barrier(0);
      const double e0 = fma(-pn, rn, 1.0);
      fmac_self_range_nn<k, 0, B / 2>(Or, nmp);
      __builtin_amdgcn_sched_barrier(0);
      rn = fma(e0, rn, rn);
      fmac_self_range_nn<k, B / 2, B>(Or, nmp);
      __builtin_amdgcn_sched_barrier(0);
      const double e1 = fma(-pn, rn, 1.0);
      fmac_self_range_nn<k, 0, B / 2>(Fr, nmp);
      __builtin_amdgcn_sched_barrier(0);
      rn = fma(e1, rn, rn);
      fmac_self_range_nn<k, B / 2, B>(Fr, nmp);
      fmac_self1_nn<k>(gr, nmp);
      __builtin_amdgcn_sched_barrier(0);
      inv = rn;
    });
    // a pivot that is not positive (or not a number) leaves a reciprocal that is not positive in its own lane: one test per
    // block step instead of one per pivot (lanes without a row keep 1)
    if (!(invs > 0.0) && live) *a.flag = 1;
    __builtin_amdgcn_sched_barrier(0);
    fused_step_prio<B>(2 * t + 1);
    GPS_TRE(49);
#pragma unroll
    for (int k = 0; k < B; k++) { Or[k] *= invs; Fr[k] *= invs; }
    gr *= invs;
    if (rowlane) {
#pragma unroll
      for (int k = 0; k < B; k++) {
        OUTR[oc + k * B] = Fr[k];
        OUTR[oc + B * B + k * B] = Or[k];
      }
      OUTR[oc + 2 * B * B] = gr;
    }
    GPS_TR(3 + min(t, 50));
    lds_barrier();                       // step t
    GPS_TRE(50);
    V2 pc[NV];
#pragma unroll
    for (int q = 0; q < NV; q++) pc[q] = *reinterpret_cast<const V2 *>(&OUTR[po + 32 * (q * 16 + r < NPC ? q : 0)]);
    double Dn[B], Fn[B], gn;
#pragma unroll
    for (int k = 0; k < B; k++) Dn[k] = nxt[ro + k];
    gn = nxt[co + 2 * B * BP];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < B; k++) Fn[k] = 0.0;
    dpp_guard();
    static_for<0, B>([&](auto ii) {
      constexpr int i = decltype(ii)::value;
      const double ol = Ol[i], gg = Gr[i];          // subtracted: the negation is the instructions' source modifier
      fmac_bcast_n_nn<i, B, true>(Fn, Fr, ol);      // F_{j+1} -= O_j[r][i] * (row i of V_j)
      fmac_bcast_n_nn<i, B, true>(Ar, Fr, gg);      // D_sep   -= G_j[r][i] * (row i of V_j)
      fmac_bcast1_nn<i, true>(gn, gr, ol);          // g_{j+1} -= O_j[r][i] * Y_j[i]
      fmac_bcast1_nn<i, true>(as_, gr, gg);         // g_sep   -= G_j[r][i] * Y_j[i]
      __builtin_amdgcn_sched_barrier(0);
    });
#pragma unroll
    for (int k = 0; k < B; k++) asm volatile("" : "+v"(Fn[k]), "+v"(Ar[k]));
    asm volatile("" : "+v"(gn), "+v"(as_));
    __builtin_amdgcn_sched_barrier(0);
    GPS_TRE(51);
    if (live) {
      V2 *dst = reinterpret_cast<V2 *>(a.blk + (size_t)j * BS);
#pragma unroll
      for (int q = 0; q < NV; q++) {
        const int idx = q * 16 + r;
        if (idx < NPC) dst[idx] = pc[q];             // (nontemporal: the iteration +3 us at 1e5 states)
      }
    }
    // G_{j+1} = F_{j+1}^T by a transpose through LDS (the V area of the factor image: its pieces were read above, and the DS
    // operations of a wave execute in order) instead of the recurrence G_{j+1} = -G_j U_j: 24 LDS operations for 144 multiply-adds
    if (rowlane) {
#pragma unroll
      for (int k = 0; k < B; k++) OUTR[tr + k] = Fn[k];
    }
    wave_lds_sync();
    double Gn[B], On[B];
#pragma unroll
    for (int k = 0; k < B; k++) { Gn[k] = OUTR[tc + k * BP]; On[k] = nxt[co + B * BP + k * BP]; }
    __builtin_amdgcn_sched_barrier(0);
    GPS_TRE(52);
    dpp_guard();
    static_for<0, B>([&](auto ii) {
      constexpr int i = decltype(ii)::value;
      fmac_bcast_n_nn<i, B, true>(Dn, Or, Ol[i]);   // D~_{j+1} -= O_j[r][i] * (row i of U_j)
      __builtin_amdgcn_sched_barrier(0);
    });
#pragma unroll
    for (int k = 0; k < B; k++) asm volatile("" : "+v"(Dn[k]));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < B; k++) { Dr[k] = Dn[k]; Fr[k] = Fn[k]; Gr[k] = Gn[k]; Or[k] = On[k]; }
    gr = gn;
    wave_lds_sync();
    __builtin_amdgcn_sched_barrier(0);
    GPS_TRE(53);
    if (!tail && live && lastb && rowlane) {
      double *ub = a.up_blk + (size_t)c * BS;
#pragma unroll
      for (int k = 0; k < B; k++) {
        ub[r * B + k] = Ar[k];
        ub[B * B + r * B + k] = right_exists ? Fr[k] : 0.0;
      }
      ub[2 * B * B + r] = as_;
      if (right_exists) {
        double *ua = a.up_add + (size_t)(c + 1) * AS;
#pragma unroll
        for (int k = 0; k < B; k++) ua[r * B + k] = Dr[k];   // -O U + R^T R of the chunk's last rows
        ua[B * B + r] = gr;
      }
    }
  }
  GPS_TR(59);
  if (!tail) { leave(); return; }

  // ================================================================== the level of groups of four, in place
  // All four chunks ended in the same block step (padding above); row grp holds what the in-loop branch above would have
  // sent to memory: the separator's record [Ar | Fr | as_] and the addend [Dr | gr] it owes the next separator.  Both
  // images are dead (the assembly wave is past its last write), they now hold the group: REC[0..3] the records, REC[4] the
  // virtual block beyond the group, TA[0..3] the addends.
  {
    constexpr int G4 = 4;
    double *REC = IMG, *TA = IMG + (G4 + 1) * BS;
    const int c0 = blockIdx.x * 4;
    const int cnt = min(G4, nch - c0);
    wave_lds_sync();
    if (valid && rowlane) {
      double *rc = REC + grp * BS, *ta = TA + grp * AS;
#pragma unroll
      for (int k = 0; k < B; k++) {
        rc[r * B + k] = Ar[k];
        rc[B * B + r * B + k] = right_exists ? Fr[k] : 0.0;
        ta[r * B + k] = Dr[k];
      }
      rc[2 * B * B + r] = as_;
      ta[B * B + r] = gr;
    }
    wave_lds_sync();
    if (valid && rowlane && grp >= 1) {          // block i >= 1 of the group receives what chunk i - 1 owes it
      double *rc = REC + grp * BS;
      const double *ta = TA + (grp - 1) * AS;
#pragma unroll
      for (int k = 0; k < B; k++) rc[r * B + k] += ta[r * B + k];
      rc[2 * B * B + r] += ta[B * B + r];
    }
    if (grp == 0 && rowlane) {                   // the block beyond the group is owed the last chunk's addend
      const bool have = (c0 + cnt < nch);
      double *rc = REC + G4 * BS;
      const double *ta = TA + (cnt - 1) * AS;
#pragma unroll
      for (int k = 0; k < B; k++) {
        rc[r * B + k] = have ? ta[r * B + k] : 0.0;
        rc[B * B + r * B + k] = 0.0;
      }
      rc[2 * B * B + r] = have ? ta[B * B + r] : 0.0;
    }
    wave_lds_sync();
    // two sub-levels: pairs (0, 1), (2, 3) on two DPP rows each (CrStepWide), then the pair (0, 2) on all four (CrStepQuad) --
    // the wave is alone in its workgroup by now, every multiply-add it does not issue is time off the launch (round 4: one row
    // per pair had cost 2 x 834 multiply-adds per lane, this is 612 + 336)
    auto sub_level = [&](int q, auto form) {
      constexpr bool quad = decltype(form)::value;
      const int h = 1 << q;
      const int pq = quad ? 0 : (grp >> 1), role4 = quad ? grp : (grp & 1);
      const int sq = pq * 2 * h, jq = sq + h;
      const bool act = jq < cnt;
      const int nq = (jq + h < cnt) ? jq + h : G4;
      std::conditional_t<quad, CrStepQuad<B>, CrStepWide<B>> st;
      if (__ballot(act) != 0ull) {               // (idle DPP rows recompute block 0; they never store)
        const bool bad = st.compute(REC, act ? sq : 0, act ? jq : 0, r, rr, role4);
        if (bad && act) *a.flag = 1;
      }
      wave_lds_sync();
      if (act && rowlane) st.store_own(REC, sq, jq, r, role4);
      wave_lds_sync();
      if (act && rowlane) {
        if constexpr (quad) { if (role4 < 2) st.add_right(REC, nq, r, role4); }
        else { if (role4 == 0) st.add_right(REC, nq, r); }
      }
      wave_lds_sync();
    };
    sub_level(0, std::false_type{});
    sub_level(1, std::true_type{});
    {   // the factor records of the eliminated separators (blocks 1 .. cnt - 1): level 1's back-substitution reads them
      V2 *dst = reinterpret_cast<V2 *>(a.l1_blk + (size_t)(c0 + 1) * BS);
      const V2 *src = reinterpret_cast<const V2 *>(REC + BS);
      for (int t = lane; t < (cnt - 1) * NPC; t += 64) dst[t] = src[t];
    }
    V2 *ub = reinterpret_cast<V2 *>(a.up_blk + (size_t)blockIdx.x * BS);
    const V2 *s0 = reinterpret_cast<const V2 *>(REC);
    for (int t = lane; t < NPC; t += 64) ub[t] = s0[t];
    V2 *ua = reinterpret_cast<V2 *>(a.up_add + (size_t)(blockIdx.x + 1) * AS);
    const V2 *s4 = reinterpret_cast<const V2 *>(REC + G4 * BS);
    for (int t = lane; t < B * B / 2 + B / 2; t += 64) ua[t] = s4[t < B * B / 2 ? t : t + B * B / 2];
  }
  GPS_TR(60);
  leave();
}

// ---------------------------------------------------------------- row-layout back-substitution (single right-hand side)
//
// k_chunk_backward_rows (round 4): the back-substitution of chains without landmark columns in the row layout of the forward
// kernels -- four chunks per wave, one per 16-lane DPP row, lane r < B holds ROW r of U_j and V_j and component r of every
// solution.  x_j = Y_j - U_j x_(j+1) - V_j x_sep is 2 B multiply-adds per lane with the solution of the state to the right
// broadcast inside the row (v_fmac_f64_dpp row_newbcast); V_j x_sep does not depend on the recurrence and is formed while the
// previous state's result is still in flight.  No LDS, no barriers: the record's 2 B + 1 operands per lane come straight from
// memory (for every q the B lanes of a row read B consecutive doubles of the column-major record [V | U | Y]), PF records ahead.
// The generic kernel above spends a wave per chunk on 12 active lanes and two LDS round trips per state: 4.2 TB/s at block size
// 12 and 2.9 TB/s at block size 6 (profiles/round4_v1, round4_c2_1e6_v1) where a streaming read reaches 5 - 6.
template <int B>
__global__ void __launch_bounds__(64) k_chunk_backward_rows(BwdArgs<double> a) {
  constexpr int BS = 2 * B * B + B;                 // R == 1
  constexpr int PF = (B == 12) ? 3 : 4;             // records in flight per chunk (vmcnt counts to 63: 3 x 25 and 4 x 13 loads, with the consumed slot excluded, stay below)
  const int lane = threadIdx.x, grp = lane >> 4, r = lane & 15;
  const int nch = (a.n + a.m - 1) / a.m;
  const int c = blockIdx.x * 4 + grp;
  const bool valid = c < nch;
  const int cc = valid ? c : 0;
  const int s = cc * a.m;
  const int e = min(s + a.m, a.n);
  const bool rowlane = r < B;
  const int rr = rowlane ? r : 0;
  const bool has_sep = !a.no_sep;
  const bool right_exists = has_sep && ((e < a.n) || (a.last_has_right != 0));
  double xs, xn;
  if (a.l1_blk != nullptr) {
    // The four separators of the wave are a group of the level above: x_0 and x_4 (the next group's first block, or zero behind
    // the chain) come from one level further up, x_2 = Y_2 - U_2 x_4 - V_2 x_0, then x_1 = Y_1 - U_1 x_2 - V_1 x_0 and
    // x_3 = Y_3 - U_3 x_4 - V_3 x_2 (cr_group_backward for G = 4; a block without a right neighbour inside the group takes x_4).
    // DPP row i holds record i of the group (25 operands per lane); two passes of one instruction stream -- the first is row 2's
    // x_2, the second rows 1 and 3 with their own operands -- and the results change rows through ds_bpermute.
    const int g = blockIdx.x, cnt = min(4, a.l1_n - 4 * g);
    const bool have = 4 * g + cnt < a.l1_n;
    const double x0 = rowlane ? a.l1_xup[(size_t)g * B + rr] : 0.0;
    const double x4 = (have && rowlane) ? a.l1_xup[(size_t)(g + 1) * B + rr] : 0.0;
    double rec[2 * B + 1];
    {
      const double *rp = a.l1_blk + (size_t)(4 * g + min(max(grp, 1), max(cnt - 1, 0))) * BS + rr;
#pragma unroll
      for (int q = 0; q < 2 * B; q++) rec[q] = rp[q * B];
      rec[2 * B] = rp[2 * B * B];
    }
    auto solve = [&](double xr, double xl) {                 // Y - U xr - V xl, summed in cr_group_backward's order
      double v = rec[2 * B];
      const double nl = -xl, nr = -xr;
      static_for<0, B>([&](auto qq) { constexpr int q = decltype(qq)::value; fmac_bcast1<q>(v, nr, rec[B + q]); });
      static_for<0, B>([&](auto qq) { constexpr int q = decltype(qq)::value; fmac_bcast1<q>(v, nl, rec[q]); });
      return v;
    };
    const double va = solve(x4, x0);                         // row 2: x_2
    const double x2 = __shfl(va, 32 + r, 64);
    const double vb = solve(grp == 1 ? ((2 < cnt) ? x2 : x4) : x4, grp == 3 ? x2 : x0);   // row 1: x_1, row 3: x_3
    const double x1 = __shfl(vb, 16 + r, 64), x3 = __shfl(vb, 48 + r, 64);
    // chunk grp of the group: its separator is block grp, the state right of it block grp + 1 (x_4 behind the group's last)
    xs = grp == 0 ? x0 : (grp == 1 ? x1 : (grp == 2 ? x2 : x3));
    xn = (grp + 1 < cnt) ? (grp == 0 ? x1 : (grp == 1 ? x2 : x3)) : x4;
    xs = (has_sep && rowlane) ? xs : 0.0;
    xn = (right_exists && rowlane) ? xn : 0.0;
  } else {
    xs = (has_sep && rowlane) ? a.xup[(size_t)cc * B + rr] : 0.0;                 // the chunk's own separator
    xn = (right_exists && rowlane) ? a.xup[(size_t)(cc + 1) * B + rr] : 0.0;      // the state right of the chunk
  }
  if (valid && rowlane) {
    if (has_sep) a.x[(size_t)s * B + r] = xs;
    // the right separator of the last chunk lives on the next rank: park its solution in the extra slot x[n]
    if (right_exists && e == a.n) a.x[(size_t)a.n * B + r] = xn;
  }
  const int j0 = has_sep ? s + 1 : s;
  const int steps = __builtin_amdgcn_readfirstlane(valid ? max(e - j0, 0) : 0);   // lane 0: the wave's first (never shorter) chunk
  if (steps <= 0) return;
  const int jlo = min(j0, e - 1);
  const int dump_off = (a.n + 1) * B + lane;       // 64 values behind the solutions (and the neighbour rank's slot): lanes without a row
  const double nxs = -xs;
  double ring[PF][2 * B + 1];
  // unconditional loads (record index clamped into the chunk): steps past a shorter chunk's first record recompute harmlessly
  auto arm = [&](int u, int j) {
    const double *rec = a.blk + (size_t)max(min(j, e - 1), jlo) * BS + rr;
#pragma unroll
    for (int q = 0; q < 2 * B; q++) ring[u][q] = rec[q * B];          // V[r][q] (q < B), U[r][q - B]
    ring[u][2 * B] = rec[2 * B * B];                                   // Y[r]
  };
  // (slot by slot, in consumption order: vmcnt counts in issue order, and the wait in front of the loop's first product is placed
  //  for the worse of its two predecessors -- with the scheduler free to interleave these loads it was vmcnt(0) on every trip)
#pragma unroll
  for (int u = 0; u < PF; u++) { arm(u, e - 1 - u); __builtin_amdgcn_sched_barrier(0); }
  for (int base = 0; base < steps; base += PF) {
#pragma unroll
    for (int u = 0; u < PF; u++) {
      const int j = e - 1 - base - u;
      // x_j = Y_j + V_j (-x_sep) + U_j (-x_(j+1)): the record's operands are consumed in load order, Y first
      double av = ring[u][2 * B], au = 0.0;
      const double nxn = -xn;
      static_for<0, B>([&](auto qq) {                // V_j x_sep: independent of the recurrence
        constexpr int q = decltype(qq)::value;
        fmac_bcast1<q>(av, nxs, ring[u][q]);
      });
      static_for<0, B>([&](auto qq) {                // U_j x_(j+1)
        constexpr int q = decltype(qq)::value;
        fmac_bcast1<q>(au, nxn, ring[u][B + q]);
      });
      double v = av + au;
      asm volatile("" : "+v"(v));                    // (formed here, not sunk into the loop latch)
      // the slot's operands are consumed: refill it (issued here, not before the products -- a refill in front of them makes the
      // compiler rotate the ring by register copies, and a copy of a register whose load is in flight drains vmcnt)
      arm(u, j - PF);
      const bool live = j >= j0;                     // (a shorter chunk of the wave is done: keep its last solution, store nothing new)
      xn = live ? v : xn;
      // unconditional, branch-free store (a store or an address under a branch breaks the wait-count bookkeeping: vmcnt(0) at the
      // next operand): finished chunks rewrite their first interior solution with the value it already has, lanes without a
      // row store to a dump
      const int off = (valid && rowlane && e > j0) ? max(j, jlo) * B + rr : dump_off;     // (a chunk that is only its separator stores nothing; n B < 2^31)
      a.x[off] = xn;
    }
  }
}

}  // namespace gps
