// api_common.hpp -- what the translation units of the library's host side share (api.hip: the C ABI; api_impl64.hip / api_impl32.hip:
// api_impl.inc + api_iterate.inc once per row precision; closures.hip, fixedlag.hip, the four marginals*.hip, dogleg.hip, evidence.hip,
// qc_learn.hip, sampling.hip, meas_noise.hip, fatsep.hip): the handle and the host helpers.  This file launches no kernel, so including it compiles none: a unit holds the
// kernels its own launch statements name (level0.hip: the level-0 row and fused forms, behind kernels.hpp's declarations; fatsep.hip: the
// segmented landmark elimination, the one includer of fatsep.hpp -- everybody else sees fatsep_plan.hpp, the plan without a kernel).
// The marginals' state is marginals.hpp's (h->mg); device buffers free themselves (devbuf.hpp: no list names them)
// (round 3: api.hip was one 3.5-minute translation unit; the fp64 and fp32 halves compile side by side now)
#pragma once
// api.hip -- host side of libgpslam_hip.so: the opaque handle, the graph-compile pass and the C ABI
// declared in include/gpslam_hip.h.  No CPU fallback exists anywhere in this library: every compute entry
// point launches HIP kernels and fails with GPSLAM_E_HIP if the device is unusable.
#include "../../include/gpslam_hip.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "devbuf.hpp"
#include "kernels.hpp"
#include "closures.hpp"
#include "marginals.hpp"
#include "fatsep_plan.hpp"
#include "upper.hpp"

using namespace gps;

namespace {

struct Level {
  int n = 0, m = 0, nch = 0;
  DevBuf blk, add, x;
};

struct SimpleSet {  // PriorFactor / BetweenFactor style factors: index + measurement + sigmas
  std::vector<int32_t> idx;
  std::vector<double> meas, sig;
  int width = 0;  // doubles per measurement
  DevBuf d_idx, d_meas, d_sig, d_row0;
  int count() const { return (int)idx.size(); }
};

struct MeasSet {  // measurement factors (kernels.hpp FKind)
  int kind = 0, rows = 1, mw = 1;
  bool two = false, haslm = false, interp = false;
  std::vector<int32_t> idx, lm;
  std::vector<double> meas, sig, dt, tau;
  // body_P_sensor / Cal3_S2 per factor: a table of distinct kMeasAux-wide entries and one index per factor
  std::vector<double> aux;
  std::vector<int32_t> aidx;
  bool any_aux = false;                // some factor of this kind carries a sensor transform or a calibration
  // noiseModel::Gaussian on factors of this kind (gpslam_hip_set_meas_covariance): rows x rows square-root information per
  // factor, diag(1 / sigma) for those that kept their diagonal model; empty: every factor is diagonal
  std::vector<double> sqi;
  // noiseModel::Robust on factors of this kind (gpslam_hip_set_meas_robust): (loss, k) per factor, (0, 0) for those without a loss;
  // empty: no factor carries one, and the kernels run as they always did
  std::vector<double> rob;
  DevBuf d_idx, d_lm, d_meas, d_sig, d_coef, d_row0, d_aux, d_aidx, d_sqi;
  DevBuf d_rob, d_w;                   // the loss table and the weights w(r) of the last pass that was asked for them
  DevBuf d_irow0;                      // first row of each factor in the table of 16-double interpolated rows (Plan::lines)
  int count() const { return (int)idx.size(); }
};

// loop closures (gpslam_hip_add_between_pairs; closures.hpp, launched by closures.hip): fac.idx = first state, second = second state
struct Closures {
  SimpleSet fac;
  std::vector<int32_t> second;
  DevBuf d_second, A, Y;
  std::vector<double> rob;            // noiseModel::Robust on closures (gpslam_hip_set_between_pairs_robust): as MeasSet::rob
  DevBuf d_rob, w;
  int n = 0, nc = 0;          // closures of the compiled graph, their right-hand-side columns (n * d)
  // closures in column passes (gpslam_hip_set_closure_passes; closures.hpp CloPass): the caller's two numbers, and what compile() made
  // of them -- P > 1: slices of `slice` closures, W = U [X | Z] and pass 0's X kept between the passes
  int max_passes = 1, per_pass = 0, slice = 0, P = 0;
  DevBuf W, X;
};

// joint Gaussian factors on one state (gpslam_hip_add_state_gaussians; fixedlag.hip): r = A [Local(pose_lin, pose_i) ; vel_i - vel_lin] - c,
// b full-width rows [A | 0] on left state idx.  The prior gpslam_hip_marginalize_head leaves on the new state 0 is one of them
struct StateGauss {
  std::vector<int32_t> idx;
  std::vector<double> lin;     // per factor [pose_lin (pd) | vel_lin (d)]
  std::vector<double> A, c;    // per factor b x b row-major, b
  DevBuf d_idx, d_lin, d_A, d_c, d_row0;
  int count() const { return (int)idx.size(); }
  void clear() { idx.clear(); lin.clear(); A.clear(); c.clear(); }
};

// joint Gaussian factors on one state AND every landmark of the handle (gpslam_hip_add_border_gaussians; fixedlag.hip): n = b + nl,
// r = A [Local(pose_lin, pose_i) ; vel_i - vel_lin ; l - lm_lin] - c.  They have no rows in the tables (a row names one landmark):
// their blocks go into record idx behind the assembly and into the landmark Schur complement behind its reduction.  The prior
// gpslam_hip_marginalize_head leaves on a handle with landmarks (gpslam_hip_marginalize_head_onto_landmarks) is one of them
struct BorderGauss {
  int nl = 0;                  // landmark coordinates of the stored factors (the handle's L * landmark_dim when they were added)
  std::vector<int32_t> idx;
  std::vector<double> lin;     // per factor [pose_lin (pd) | vel_lin (d) | lm_lin (nl)]
  std::vector<double> A, c;    // per factor n x n row-major, n
  DevBuf d_idx, d_lin, d_A, d_c, d_r;   // d_r: count x n residuals of the last pass
  int count() const { return (int)idx.size(); }
  void clear() { idx.clear(); lin.clear(); A.clear(); c.clear(); nl = 0; }
};

// Which kernels serve a compiled graph, and in which form.  make_plan() (api_impl.inc) fills one per compile(), once the row layout
// is known, and nothing else writes it; what a single launch then does is launch_form(handle, LaunchMode) below.
enum class Level0 { Column, Rows, Fused };     // level-0 elimination: k_chunk_forward, k_chunk_forward_rows, or k_fused_level0 where the mode asks for it
enum class GpForm { Rows, Se3Rec, D3Rec };     // GP priors as Jacobian rows, as SE(3) records (kGps*: GpArgs::gps -> k_fused_level0) or as d = 3
                                               // records (kGp3*: block size 6, which k_assemble_ghost decodes as well)
struct Plan {
  Level0 level0 = Level0::Column;
  bool upper_cr = false;        // the levels above level 0 run as LDS-resident cyclic reduction (upper.hip)
  GpForm gp_rec = GpForm::Rows; // the form a launch that carries records uses
  bool btw_rec = false;         // BetweenFactor<Pose3> rides with the SE(3) records as 48-double records (kBtw*): at most one per left state
  bool lines = false;           // SE(3) records + interpolated GPS rows as 16-double lines (k_gps_lines -> k_fused_level0<4>): every
                                // full-width row besides the GP priors' belongs to such a factor on an interval that has a GP prior
  int odd_rows = 0;             // full-width rows besides the GP priors': 0 none, 1 a few (k_fused_level0<2> fetches them without a ring), 2 many (<3>)
  bool pure6 = false;           // block size 6: next to nothing but d = 3 GP records in the full-width table (fused level 0 at every size)
  bool fold_retract = false;    // run_gn folds an iteration's retraction into the next iteration's K1 (kernels.hpp: PendUpd)
  // level 1 as groups of four: a fused level 0 reduces them in its own tail, k_chunk_backward_rows solves its group itself
  bool tail_fold = false, fold_tail_bwd = false;
  // the row placement the record decoders rely on (checks, not options: without them the record forms above are off)
  bool gp_rows_lead = true, btw_rows_trail = true;
  bool rows() const { return level0 != Level0::Column; }
  bool fused() const { return level0 == Level0::Fused; }
};

}  // namespace

// gpslam_hip_launch_census: what the launchers did since the last reset (GPSLAM_CENSUS_*).  Host-side integers, written at the launch
// statements from the branch taken -- never derived from the plan or from launch_form()
struct LaunchCensus {
  int32_t v[GPSLAM_CENSUS_N];
  LaunchCensus() { clear(); }
  void clear() {   // counts to 0, the entries that describe the last k_fused_level0 launch to "none"
    for (int i = 0; i < GPSLAM_CENSUS_N; i++) v[i] = (i >= GPSLAM_CENSUS_FUSED_SV && i <= GPSLAM_CENSUS_FUSED_TAIL) ? -1 : 0;
  }
  int32_t &operator[](int i) { return v[i]; }
};

// gpslam_hip_iterate_dogleg (dogleg.hip): the landmark gradient g_L and the landmarks' part of the Gauss-Newton step (the states' parts
// are gsave and dvec), the partial sums of g^T H g and g . g, and what the last call computed (gpslam_hip_dogleg_last)
struct Dogleg {
  DevBuf gL, nL, part;
  double last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// gpslam_hip_log_determinant (evidence.hip): the separators' systems of the levels above 0 (three blocks each: D, O, add), one
// partial sum of log-pivots per chunk of every level, and what the call reads back ({log det A, log det(I + U Z), log det S, flag})
struct Evidence {
  int N = 0;                  // the N the buffers are sized for
  DevBuf up, part, res;
  // the buffers serve n states from here on: another N frees what is there (as Marginals::fit)
  void fit(int n) {
    if (N != n) { up.release(); part.release(); }
    N = n;
  }
};

// gpslam_hip_qc_statistic (qc_learn.hip): one d x d partial sum per workgroup of k_qc_stat, and the d x d result behind them
struct QcLearn {
  int N = 0;                  // the N the buffer is sized for
  DevBuf part;
  // the buffer serves n states from here on: another N frees what is there (as Marginals::fit)
  void fit(int n) {
    if (N != n) part.release();
    N = n;
  }
};

// gpslam_hip_sample_posterior (sampling.hip): a chunk of noise rows, the scratch copy of the landmark priors' measurements that stands
// in for lpri.d_meas during a call, the tables' whitened errors as the call's linearisation left them, and the output slabs of a chunk
struct Sampling {
  DevBuf stage, pri, saveE;
  DevBuf delta, poses, vels, lms;
  // gpslam_hip_sample_posterior_at: a call's query runs (CSR over runs: first query of each, its interval), the eleven bridge
  // coefficients of every query, and the query slabs of a chunk
  DevBuf at_ptr, at_left, at_coef;
  DevBuf at_poses, at_vels;
  // gpslam_hip_sample_posterior_stats: a call's q^ with the interpolators' tables it comes from, its obstacles, the per-query sums,
  // and per chunk the clearance and segment slabs with the per-draw numbers they reduce to
  DevBuf st_ref, st_left, st_coef, st_obs;
  DevBuf st_s1, st_s2, st_hits;
  DevBuf st_g, st_seg, st_part, st_clear, st_len;
};

// gpslam_hip_meas_noise_statistic / gpslam_hip_meas_predicted_covariances (meas_noise.hip): per kind the factors' order by left state
// (a stable sort inside every chunk of the pass, built on the host at the first call after a compile() and kept), the call's `use`
// bytes, one 2 r x r partial per workgroup of k_mn_stat, the first reduction stage's sums with the result behind them, and a chunk's P_m
struct MeasNoise {
  int N = 0;                  // the N the buffers are sized for
  DevBuf perm[kNumMeasKinds];
  bool have[kNumMeasKinds] = {false, false, false, false, false, false, false, false};
  DevBuf use, part, cpart, P;
  void invalidate() { for (bool &v : have) v = false; }   // compile(): the factors may be others
  // the buffers serve n states from here on: another N frees what is there (as Marginals::fit)
  void fit(int n) {
    if (N != n) {
      for (DevBuf &p : perm) p.release();
      for (DevBuf *p : {&use, &part, &cpart, &P}) p->release();
      invalidate();
    }
    N = n;
  }
};

// Work one launch leaves to a later one (chains without landmarks, unsharded: gn_mode; run_gn with Plan::fold_retract).  update: a
// solve's step sits in the level-0 solution array, not yet applied -- the next k_lin applies it (kernels.hpp: PendUpd), or
// flush_update.  err: the linearisation's error partial sums in `partial`, summed by an extra workgroup of this iteration's
// k_retract.  dmax: the retraction's |delta|_inf partial maxima in `partial2`, reduced by an extra workgroup of the NEXT iteration's
// k_lin -- two launches (+ their gaps) less per iteration, same values, same order
struct Deferred {
  bool update = false;
  struct Sums {
    int n = 0, slot = 0;      // n > 0: that many partials wait, for scal[slot]
    Sums take() { const Sums s = *this; n = 0; return s; }   // the launch that reduces them says so
  } err, dmax;
  void clear() { update = false; err.n = 0; dmax.n = 0; }
};

struct gpslam_hip_handle {
  gpslam_hip_config_v2 cfg;   // (gpslam_hip_create maps a v1 config onto it)
  int mf = 0, d = 0, pd = 0, b = 0, ld = 0;
  int vw = 0;                 // Pose3: velocities are world-frame [v; w] (cfg.velocity, the *Pose3VW factors)
  int N = 0, L = 0, stride = 0, R = 1, nl = 0;
  bool own_stream = true;
  hipStream_t stream = nullptr;
  hipStream_t aux_stream = nullptr;   // side stream for the light factor kernels (launch_factors)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_l0a = nullptr, ev_l0b = nullptr;   // the fused level-0 launch's own stamps in a timed iteration (LaunchMode::l0_events)
  bool l0_stamps = false;     // gpslam_hip_set_level0_stamps: timed iterations use them (off: events around the launch, as in rounds 1-5)
  double Qc[36], U[36];
  std::vector<double> h_lmk;
  DevBuf pose, vel, lmk, pose_bak, vel_bak, lmk_bak;
  // factors
  std::vector<int32_t> gp_left;
  std::vector<double> gp_dt;
  DevBuf d_gp_left, d_gp_dt, d_gp_row0;
  // one Qc_model per GP prior (gpslam_hip_add_gp_priors_qc; GaussianProcessPriorPose3.h:43-49): gp_q[f] = 0: the handle's
  // shared Qc (set_qc), k >= 1: entry k - 1 of gp_Utab (36 doubles each, chol_upper(Qc^-1)).  With more than one distinct
  // Qc, compile() orders the device-side factor arrays by Qc (gp_perm: device position -> position in the order added)
  // and the linearisation runs one launch per group (gp_groups: {q, first, count}), each with its U as a kernel argument.
  std::vector<int32_t> gp_q;
  std::vector<double> gp_Utab;
  std::vector<double> gp_Qtab;  // the Qc behind each entry of gp_Utab as it was given (36 doubles each, d x d leading; evidence.hip)
  std::vector<int32_t> gp_perm;
  std::vector<int32_t> gp_groups;
  int gp_single_q = 0;      // > 0: every GP prior came through add_gp_priors_qc with the SAME Qc (entry gp_single_q - 1 of gp_Utab):
                            // one group, one launch, and the structured-record path of k_fused_level0 stays available
  SimpleSet pri, vpri, btw, lpri;
  Closures clo;
  MeasSet ms[kNumMeasKinds];
  StateGauss sg;
  BorderGauss bg;
  bool fl_onto_lm = false;    // gpslam_hip_marginalize_head_onto_landmarks
  std::vector<double> hpb;    // gpslam_hip_get_head_prior_border: [lm_lin (nl) | Lambda (n x n) | gamma (n)] of the last joint marginalize_head, or empty
  int hpb_nl = 0;             // ... and its nl
  DevBuf fl_head;             // marginalize_head onto landmarks: [H_LL^head (nl x nl) | g_L^head (nl)]
  std::vector<double> hp;     // gpslam_hip_get_head_prior: [pose_lin | vel_lin | Lambda | gamma] of the last marginalize_head, or empty
  DevBuf fl_out, fl_flag;     // marginalize_head: [D_k^left | g_k^left | B_k^left | Lambda | g'_k | pose_k | vel_k | landmarks] and the recursion's flag
  // row table
  int M = 0;
  DevBuf rowLR, rowE, rowM, rowLm, rowptr;
  DevBuf partial;
  // landmark border
  int nlmrows = 0;
  DevBuf rowC, rowCE, crowptr;   // compact row table (pose priors, between factors) and its row pointers
  int Mc = 0;
  DevBuf lmrow, lmrow_state, lmrow_ptr, lm_t, lm_S, lm_dL;   // lm_S = [S (nl x R) | gL (nl)]
  DevBuf lm_chunk_lm, lm_chunk_j0, lm_chunk_j1, lm_chunk_ptr, lm_part;   // chunked reduction of the landmark rows
  int nlmchunks = 0;
  // solver
  std::vector<Level> lv;
  DevBuf gsave, dvec;
  // segment sharding
  DevBuf halo_add, iface_send, iface_recv, top_blk, top_x;
  DevBuf scal, flag, api_e, api_H;
  // landmark elimination at scale (fatsep_plan.hpp; fatsep.hip): segments + fat separators instead of the dense border
  FatSepPlan fs;
  DevBuf lm_gL;             // undamped landmark gradient of the segmented path (the dense path keeps it behind lm_S)
  Plan plan;                // compile(): which kernels serve this graph, in which form
  LaunchCensus census;      // gpslam_hip_launch_census
  DevBuf gps, gpidx, dU, gsave2;
  DevBuf simd_cnt;          // k_fused_level0 (role swap): wave-0 count per SIMD of the chip, zero between launches
  DevBuf rowI, irowptr;     // Plan::lines
  // the host's collectives (gpslam_hip_set_collectives): with them the optimiser loops run on sharded handles / split pieces
  gpslam_hip_all_gather_fn coll_gather = nullptr;
  gpslam_hip_all_reduce_sum_fn coll_reduce = nullptr;
  void *coll_user = nullptr;
  DevBuf coll_s, coll_r;     // 8 doubles of this rank's scalars, nranks x 8 gathered
  DevBuf brec, btwidx;      // Plan::btw_rec
  // set_qc after compile(): refresh_dU brings the device copy of U (and U_diag) up to date before a launch reads it
  int U_version = 0, dU_version = -1;
  bool U_diag = false;        // the U in dU is diagonal (an isotropic or diagonal Qc): the SE(3) record variants take the shorter assembly form
  bool compiled = false;
  double last_ms[5] = {0, 0, 0, 0, 0};
  DevBuf partial2;            // the retraction's per-block maxima (its own buffer: the linearisation reuses `partial`)
  Deferred defer;
  double l0_ms = 0.0;         // the level-0 forward launch, accumulated over the last timed run: the dominant kernel INSIDE an iteration
  double ph_lambda = 0.0;
  Marginals mg;               // gpslam_hip_marginals (marginals.hpp): what the last call left; every call that can change states, landmarks,
                              // factors or Qc says h->mg.invalidate()
  Dogleg dl;                  // gpslam_hip_iterate_dogleg (dogleg.hip)
  Evidence evd;               // gpslam_hip_log_determinant (evidence.hip)
  QcLearn qcl;                // gpslam_hip_qc_statistic (qc_learn.hip)
  Sampling ps;                // gpslam_hip_sample_posterior (sampling.hip)
  MeasNoise mn;               // gpslam_hip_meas_noise_statistic (meas_noise.hip)
  std::string err;
#ifdef GPS_TRACE_FUSED
  DevBuf dbg_trace;           // debug builds only: 64 stamps per wave of the last k_fused_level0 launch
  int dbg_trace_waves = 0;
#endif
};

// What the launches of one call do: each entry point builds the mode it means and hands it to the launch helpers.
// LaunchMode{}: row tables (d = 3 records where the graph has them), level 0 unfused, every reduction at once, untimed.
struct LaunchMode {
  bool fused = false;         // level 0 runs as k_fused_level0 (the assembly inside the elimination)
  bool se3_rec = false;       // the SE(3) GP priors travel as structured records (linearisation -> k_fused_level0)
  bool d3_rows = false;       // the d = 3 GP priors as rows after all, not as kGp3* records (gpslam_hip_get_rows: the table is wanted)
  bool gsave = false;         // k_fused_level0 stores the gradient (Levenberg-Marquardt trials)
  bool defer_error = false;   // the linearisation leaves its error partial sums to the extra workgroup of this iteration's k_retract
  bool defer_maxima = false;  // the retraction leaves its |delta|_inf partial maxima to the next iteration's k_lin
  bool stamp_l0 = false;      // a timed iteration also stamps the end of the level-0 forward launch (ev[5])
  // ... and the fused level-0 launch carries its own start / stop events (hipExtLaunchKernelGGL: the dispatch's own time stamps,
  // what rocprofv3's kernel trace reads) -- events recorded AROUND a launch add their marker packets to it (7 us of 149)
  bool l0_events = false;
  bool weights = false;       // an error-only pass that also stores every robust factor's weight w(r) (MeasArgs::out_w, CloArgs::out_w)
  bool keep_z = false;        // launch_solve in column passes: every pass's slice of Z = A^-1 U^T into h->mg.Z (the marginals)
  bool lm_reduce_only = false;   // launch_solve ends with the landmark Schur complement, without the landmark solve (the states stay)
};

// Loop closures (closures.hip; fp64 only: both precision namespaces call these, and compile() refuses closures on an fp32 handle).
// closures_upload: compile()'s share -- the factor set to the device, the buffers sized.  closures_eval: the records [A_i | A_j | r]
// (pass 0) and the closures' error into partial[0], on stream st.  closures_inject: behind the assembly, slice `pass` of the columns
// of U^T into the records (U^T r into the gradient copy if save_g); pass == P in column passes: the final pass's right-hand sides
// U^T Y.  closures_correct: one pass -- Y = (I + U Z)^-1 ([r | 0] - U X) and X += Z Y, between the chain's back-substitution and the
// landmark Schur complement.  Column passes (launch_solve_passes, api_impl.inc): closures_collect behind pass p's backward sweep
// (keep_z: the slice of Z into h->mg.Z first; pass 0: X saved; W gathered; behind the last pass the wide solve for Y),
// closures_add behind the final pass.
int closures_upload(gpslam_hip_handle *h);
void closures_eval(gpslam_hip_handle *h, const LaunchMode &m, int pass, double *partial, hipStream_t st);
void closures_inject(gpslam_hip_handle *h, bool save_g, int pass);
int closures_correct(gpslam_hip_handle *h);
void closures_collect(gpslam_hip_handle *h, int p, bool keep_z);
int closures_add(gpslam_hip_handle *h);
// row length of W = U [X | Z] (CloPass::ldw)
inline int clo_ldw(const gpslam_hip_handle *h) { return 1 + h->nl + h->clo.nc; }

// The segmented landmark elimination (fatsep.hip: the one unit that includes fatsep.hpp's kernels).  The Jacobian rows' type is chosen
// inside, once per call, from the handle's precision; both precision namespaces and marginals_fs.hip call these.  fs_build: compile()'s
// share -- segment plan, level sets of the cyclic reduction, buffers, the dynamic-LDS attributes of the handle's row type (touch_lo /
// touch_hi: first / last state touched by the factors of each landmark).  fs_forward: segment interiors -> fat blocks -> the
// cyclic-reduction levels, down to one block or to the two end blocks of a piece of a split chain (y_own: the sweep and the Schur
// complements in two launches through THIS Y buffer, whatever the plan's choice).  fs_solve: the whole solve behind an assembly.  A
// piece of a split chain: fs_pack_record behind fs_forward (the interface record into the send buffer), fs_split_solve once the
// records of every piece are in (the top system, then the piece's backward half at h->ph_lambda).
int fs_build(gpslam_hip_handle *h, const std::vector<int> &touch_lo, const std::vector<int> &touch_hi);
int fs_forward(gpslam_hip_handle *h, double lambda, double *y_own = nullptr);
int fs_solve(gpslam_hip_handle *h, double lambda);
int fs_pack_record(gpslam_hip_handle *h);
int fs_split_solve(gpslam_hip_handle *h);
// ... and the launches that stand inside other steps, each on the stream it is given.  fs_lmprior_err: the landmark priors' error,
// nbl partial sums (launch_other_factors; an fp32 handle's error pass is the fp64 half's, so the type of the sums is the caller's).
// fs_lm_update: landmarks += dL and |dL|_inf folded into scal[slot] (launch_retract).  fs_mask_mul: dL with the landmarks a
// neighbour piece counts zeroed, into fs.lm_tmp (trial_scalars).
void fs_lmprior_err(gpslam_hip_handle *h, int nbl, double *partial, hipStream_t st);
void fs_lmprior_err(gpslam_hip_handle *h, int nbl, float *partial, hipStream_t st);
void fs_lm_update(gpslam_hip_handle *h, int slot, hipStream_t st);
void fs_mask_mul(gpslam_hip_handle *h, const double *dL, hipStream_t st);
// The segmented path sends the light factor kernels (launch_factors) and its own row-table kernels (fs_forward) to the handle's second
// stream, underneath the chain's, only on graphs of at least this many states: everywhere else everything stays on one stream.  A/B of "never"
// against "always" (scripts/ab_fork.py, wall clock of run_gn(20), ms per iteration): Plaza2 (4091 states) 0.152 / 0.192 -- its
// timeline: k_lin 7 us beside k_meas 10 us, then 12 us of nothing before the reduction starts; config 5's SO(3) mix 3e4 0.100 /
// 0.117, 1e5 0.208 / 0.213, 1e6 1.518 / 1.540; config 4's mix 1e5 0.885 / 0.916, 3e5 1.388 / 1.411, 1e6 3.019 / 2.997 -- joining two
// streams costs more idle time (12 us and up) than the shorter of two concurrent kernels saves, and two kernels side by side slow each
// other down: only the segmented landmark path (config 4's mix) at 1e6 states gains (0.7 %), and only it forks.
constexpr int kForkMinStates = 524288;

// State Gaussians (fixedlag.hip; fp64 only: compile() refuses them on an fp32 handle).  state_gauss_upload: compile()'s share (row0: the
// first row of each factor in the full-width table).  state_gauss_eval: the rows [A | 0], their error entries (pass 0) and the error
// partial sums, nblocks(count, 128) of them, on stream st.
int state_gauss_upload(gpslam_hip_handle *h, const std::vector<int> &row0);
void state_gauss_eval(gpslam_hip_handle *h, int pass, double *partial, hipStream_t st);

// Border Gaussians (fixedlag.hip; fp64 only, dense landmark border).  border_gauss_upload: compile()'s share.  border_gauss_eval: the
// residuals (pass 0 only: kept on the device as the linearisation's, an error-only pass at a trial point leaves them alone) and the
// error, one partial sum, on stream st.  border_gauss_inject: behind the assembly, A_x^T A_x,
// A_x^T (c - A xi) and A_x^T A_L into record idx (the gradient copy too if save_g).  border_gauss_schur: behind k_lm_reduce, the
// factor's share of [S | gL] -- k_lm_t forms B^T Z from the rows, and this factor has none.
int border_gauss_upload(gpslam_hip_handle *h);
void border_gauss_eval(gpslam_hip_handle *h, int pass, double *partial, hipStream_t st);
void border_gauss_inject(gpslam_hip_handle *h, bool save_g);
void border_gauss_schur(gpslam_hip_handle *h);

#define HIPCHK(call)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      h->err = std::string(#call) + ": " + hipGetErrorString(e_);                             \
      return GPSLAM_E_HIP;                                                                    \
    }                                                                                         \
  } while (0)

namespace {

int fail(gpslam_hip_handle *h, int code, const char *msg) {
  h->err = msg;
  return code;
}

bool spd_chol_upper(int n, double *A) {
  for (int j = 0; j < n; j++) {
    double dd = A[j * n + j];
    for (int k = 0; k < j; k++) dd -= A[k * n + j] * A[k * n + j];
    if (!(dd > 0.0)) return false;
    dd = std::sqrt(dd);
    A[j * n + j] = dd;
    for (int i = j + 1; i < n; i++) {
      double s = A[j * n + i];
      for (int k = 0; k < j; k++) s -= A[k * n + j] * A[k * n + i];
      A[j * n + i] = s / dd;
    }
    for (int i = 0; i < j; i++) A[j * n + i] = 0.0;
  }
  return true;
}

// U = chol_upper(Qc^-1): invert Qc through its own Cholesky factor, then factor the inverse
bool make_U(int n, const double *Qc, double *U) {
  double C[36], Ci[36], Qi[36];
  std::memcpy(C, Qc, sizeof(double) * n * n);
  if (!spd_chol_upper(n, C)) return false;  // Qc = C^T C
  std::memset(Ci, 0, sizeof(Ci));
  for (int j = 0; j < n; j++) {
    Ci[j * n + j] = 1.0 / C[j * n + j];
    for (int i = j - 1; i >= 0; i--) {
      double s = 0.0;
      for (int k = i + 1; k <= j; k++) s += C[i * n + k] * Ci[k * n + j];
      Ci[i * n + j] = -s / C[i * n + i];
    }
  }
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      double s = 0.0;
      for (int k = 0; k < n; k++) s += Ci[i * n + k] * Ci[j * n + k];
      Qi[i * n + j] = s;
    }
  std::memcpy(U, Qi, sizeof(double) * n * n);
  return spd_chol_upper(n, U);
}

// First block row of Lambda(tau), Psi(tau) (gpslam/gp/GPutils.h:54-71): [l11 I, l12 I], [p11 I, p12 I].
// Psi = Q(tau) Phi(dt - tau)^T Q^-1(dt) = (A(tau) Phi2(dt - tau)^T Ainv(dt)) (x) (Qc Qc^-1);  Lambda = Phi(tau) - Psi Phi(dt)
void interp_coef(double dt, double tau, double *out4) {
  const double s = dt - tau;
  const double a11 = tau * tau * tau / 3.0 + s * tau * tau / 2.0, a12 = tau * tau / 2.0;   // first row of A(tau) Phi2(s)^T
  const double p11 = a11 * (12.0 / (dt * dt * dt)) + a12 * (-6.0 / (dt * dt));
  const double p12 = a11 * (-6.0 / (dt * dt)) + a12 * (4.0 / dt);
  out4[0] = 1.0 - p11;
  out4[1] = tau - p11 * dt - p12;
  out4[2] = p11;
  out4[3] = p12;
}

// synchronous host -> device copy of a vector (the stream is drained so temporaries may die)
template <typename V> int upload(gpslam_hip_handle *h, DevBuf &buf, const std::vector<V> &v) {
  HIPCHK(buf.reserve(v.size() * sizeof(V)));
  if (!v.empty()) {
    HIPCHK(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}
// a SimpleSet's arrays (row0: the first row of each factor in its row table, or empty)
inline int upload_set(gpslam_hip_handle *h, SimpleSet &s, const std::vector<int> &row0) {
  int rc;
  if ((rc = upload(h, s.d_idx, s.idx)) || (rc = upload(h, s.d_meas, s.meas)) || (rc = upload(h, s.d_sig, s.sig))) return rc;
  return upload(h, s.d_row0, row0);
}
inline int nblocks(int n, int bs) { return (n + bs - 1) / bs; }

// ---- manifold / block-size dispatch: call f(std::integral_constant<int, X>{}) for the runtime value
template <typename F> void dispatch_mf(int mf, F &&f) {
  switch (mf) {
    case LINEAR2: f(std::integral_constant<int, LINEAR2>{}); break;
    case LINEAR3: f(std::integral_constant<int, LINEAR3>{}); break;
    case POSE2: f(std::integral_constant<int, POSE2>{}); break;
    case POSE3: f(std::integral_constant<int, POSE3>{}); break;
    case ROT3: f(std::integral_constant<int, ROT3>{}); break;
    case ROT3_BIAS: f(std::integral_constant<int, ROT3_BIAS>{}); break;
  }
}
template <typename F> void dispatch_b(int b, F &&f) {
  switch (b) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 12: f(std::integral_constant<int, 12>{}); break;
  }
}
template <typename F> void dispatch_fk(int fk, F &&f) {
  switch (fk) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
  }
}

// force_sharded = 1 forces the sharded code path on a single segment (self-test of the exchange plumbing)
bool sharded(const gpslam_hip_handle *h) { return h->cfg.nranks > 1 || h->cfg.force_sharded == 1; }
bool has_right_rank(const gpslam_hip_handle *h) { return sharded(h) && h->cfg.rank < h->cfg.nranks - 1; }
// a piece of a chain split at shared cut states (gpslam_hip_fs_set_split)
bool split_piece(const gpslam_hip_handle *h) { return h->fs.active && h->fs.split; }

// some measurement factor or closure carries a loss (noiseModel::Robust)
bool any_robust(const gpslam_hip_handle *h) {
  bool any = !h->clo.rob.empty();
  for (const MeasSet &s : h->ms) any = any || !s.rob.empty();
  return any;
}

bool plan_bit(const gpslam_hip_handle *h, int bit) { return (h->cfg.plan & bit) != 0; }   // GPSLAM_PLAN_*

// The one rule for level 0 of an iteration: fused where compile() found k_fused_level0 applicable, except on an unsharded
// chain of a single level (that level is the top solve; a sharded rank's level 0 always keeps its separator), and then
// with the GP priors as SE(3) records where the graph allows them.
LaunchMode level0_mode(const gpslam_hip_handle *h) {
  LaunchMode m;
  m.fused = h->plan.fused() && (h->lv.size() >= 2 || sharded(h));
  m.se3_rec = m.fused && h->plan.gp_rec == GpForm::Se3Rec;
  return m;
}

// What one launch uses, from the plan and the launch's mode -- the one place that says so.
struct LaunchForm {
  GpForm gp = GpForm::Rows;   // the GP priors on this launch
  bool btw_rec = false;       // between factors travel as records
  bool lines = false;         // interpolated GPS rows travel as 16-double lines
  int sv = 0;                 // k_fused_level0<sv, ., ., dg> (launch_fused_k)
  bool dg = false;
};
// SE(3) records when the launch says so; d = 3 records whenever the graph has them (every consumer decodes them) and the row table
// itself is not what is wanted
GpForm gp_form(const gpslam_hip_handle *h, const LaunchMode &m) {
  if (m.se3_rec && h->plan.gp_rec == GpForm::Se3Rec) return GpForm::Se3Rec;
  return (h->plan.gp_rec == GpForm::D3Rec && !m.d3_rows) ? GpForm::D3Rec : GpForm::Rows;
}
LaunchForm launch_form(const gpslam_hip_handle *h, const LaunchMode &m) {
  const Plan &p = h->plan;
  LaunchForm f;
  f.gp = gp_form(h, m);
  const bool se3 = f.gp == GpForm::Se3Rec;
  f.btw_rec = se3 && p.btw_rec;
  f.lines = se3 && p.lines;
  // records + lines: <4>; + a ring of full-width rows (measurement factors): <3>; + a few rows fetched where they are used: <2>
  f.sv = f.gp == GpForm::Rows ? 0 : (!se3 ? 1 : (f.lines ? 4 : (p.odd_rows == 2 ? 3 : (p.odd_rows == 1 ? 2 : 1))));
  f.dg = se3 && h->U_diag && !plan_bit(h, GPSLAM_PLAN_GENERIC_QC);   // (U_diag: as of refresh_dU, which every launch that reads dU calls first)
  return f;
}

int read_scal(gpslam_hip_handle *h, double *out, int n, int *flag) {
  HIPCHK(hipMemcpyAsync(out, h->scal.p, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(flag, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int collect_timing(gpslam_hip_handle *h, const LaunchMode &m, double *acc) {
  float ms;
  for (int i = 0; i < 4; i++) {
    HIPCHK(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
    acc[i] += ms;
  }
  HIPCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[4]));
  acc[4] += ms;
  if (m.stamp_l0) {             // the level-0 forward launch of this iteration: its own stamps, or (unfused) ev[2] = start of the solve phase
    if (m.l0_events) HIPCHK(hipEventElapsedTime(&ms, h->ev_l0a, h->ev_l0b));
    else HIPCHK(hipEventElapsedTime(&ms, h->ev[2], h->ev[5]));
    h->l0_ms += ms;
  }
  return 0;
}

int need_compiled(gpslam_hip_handle *h) {
  if (!h) return GPSLAM_E_INVALID;
  if (!h->compiled) return fail(h, GPSLAM_E_NOT_COMPILED, "call gpslam_hip_compile() first");
  return 0;
}
// ... and its device current: the opening of every call that works on this handle's own share of the chain, whatever the scheme
// (api_iterate.inc has the guards that also ask for a kind of handle)
int need_local(gpslam_hip_handle *h) {
  int rc = need_compiled(h);
  if (!rc) (void)hipSetDevice(h->cfg.device);
  return rc;
}

int add_simple(gpslam_hip_handle *h, SimpleSet &s, int width, int sigw, int32_t count, const int32_t *idx,
               const double *meas, const double *sig, int max_idx) {
  if (!h || count < 0 || (count > 0 && (!idx || !meas || !sig))) return GPSLAM_E_INVALID;
  for (int k = 0; k < count; k++)
    if (idx[k] < 0 || idx[k] > max_idx) return fail(h, GPSLAM_E_INVALID, "factor index out of range");
  for (size_t k = 0; k < (size_t)count * sigw; k++)
    if (!(sig[k] > 0.0)) return fail(h, GPSLAM_E_INVALID, "sigmas must be positive");
  s.width = width;
  s.idx.insert(s.idx.end(), idx, idx + count);
  s.meas.insert(s.meas.end(), meas, meas + (size_t)count * width);
  s.sig.insert(s.sig.end(), sig, sig + (size_t)count * sigw);
  h->compiled = false;
  h->mg.invalidate();
  return 0;
}

// index of the last state a two-state factor may start at (the halo state extends a non-final segment by one)
int max_left(const gpslam_hip_handle *h) { return h->N - 2 + (has_right_rank(h) ? 1 : 0); }

int add_meas(gpslam_hip_handle *h, int fk, int rows, int mw, bool two, bool haslm, bool interp, bool ok_mf,
             int32_t count, const int32_t *idx, const int32_t *lm, const double *meas, const double *sig,
             const double *dt, const double *tau, const double *sensor, const double *calib = nullptr, const double *distortion = nullptr) {
  if (!h || count < 0) return GPSLAM_E_INVALID;
  if (!ok_mf) return fail(h, GPSLAM_E_INVALID, "this factor does not exist for the handle's manifold / landmark dimension");
  if (count > 0 && (!idx || !meas || !sig || (haslm && !lm) || (interp && (!dt || !tau)))) return GPSLAM_E_INVALID;
  MeasSet &s = h->ms[fk];
  const int mx = two ? max_left(h) : h->N - 1;
  for (int k = 0; k < count; k++) {
    if (idx[k] < 0 || idx[k] > mx) return fail(h, GPSLAM_E_INVALID, "factor state index out of range");
    if (haslm && (lm[k] < 0 || lm[k] >= h->L)) return fail(h, GPSLAM_E_INVALID, "landmark index out of range (set_landmarks first)");
    if (interp && !(dt[k] > 0.0)) return fail(h, GPSLAM_E_INVALID, "delta_t must be positive");
  }
  for (size_t k = 0; k < (size_t)count * rows; k++)
    if (!(sig[k] > 0.0)) return fail(h, GPSLAM_E_INVALID, "sigmas must be positive");
  s.kind = fk; s.rows = rows; s.mw = mw; s.two = two; s.haslm = haslm; s.interp = interp;
  s.idx.insert(s.idx.end(), idx, idx + count);
  if (haslm) s.lm.insert(s.lm.end(), lm, lm + count);
  s.meas.insert(s.meas.end(), meas, meas + (size_t)count * mw);
  s.sig.insert(s.sig.end(), sig, sig + (size_t)count * rows);
  if (!s.sqi.empty()) {   // the kind already has Gaussian factors: the newcomers' diagonal models as matrices
    for (int k = 0; k < count; k++)
      for (int r = 0; r < rows; r++)
        for (int q = 0; q < rows; q++) s.sqi.push_back(r == q ? 1.0 / sig[(size_t)k * rows + r] : 0.0);
  }
  if (!s.rob.empty()) s.rob.insert(s.rob.end(), (size_t)count * 2, 0.0);   // the kind already has robust factors: the newcomers carry no loss
  if (interp) { s.dt.insert(s.dt.end(), dt, dt + count); s.tau.insert(s.tau.end(), tau, tau + count); }
  {   // this call's body_P_sensor / calibration: find it in (or append it to) the kind's table
    double ent[kMeasAux] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0};
    if (sensor) { std::memcpy(ent, sensor, sizeof(double) * h->pd); ent[17] = 1.0; }
    if (calib) std::memcpy(ent + 12, calib, sizeof(double) * 5);
    if (distortion) std::memcpy(ent + 18, distortion, sizeof(double) * 4);
    int slot = -1;
    const int nent = (int)(s.aux.size() / kMeasAux);
    for (int q = 0; q < nent && slot < 0; q++)
      if (std::memcmp(&s.aux[(size_t)q * kMeasAux], ent, sizeof(ent)) == 0) slot = q;
    if (slot < 0) { slot = nent; s.aux.insert(s.aux.end(), ent, ent + kMeasAux); }
    s.aidx.insert(s.aidx.end(), (size_t)count, slot);
    if (sensor || calib) s.any_aux = true;
  }
  h->compiled = false;
  h->mg.invalidate();
  return 0;
}

int sync_landmarks_to_host(gpslam_hip_handle *h) {
  if (h->L <= 0 || !h->lmk.p) return 0;
  std::vector<double> t((size_t)h->L * h->ld);
  HIPCHK(hipMemcpyAsync(t.data(), h->lmk.p, t.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < t.size(); i++) h->h_lmk[i] = (double)t[i];
  return 0;
}

int backup_state(gpslam_hip_handle *h, bool restore) {
  const size_t np = (size_t)h->pd * h->stride * sizeof(double), nv = (size_t)h->d * h->stride * sizeof(double);
  HIPCHK(h->pose_bak.reserve(np));
  HIPCHK(h->vel_bak.reserve(nv));
  if (restore) {
    HIPCHK(hipMemcpyAsync(h->pose.p, h->pose_bak.p, np, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->vel.p, h->vel_bak.p, nv, hipMemcpyDeviceToDevice, h->stream));
  } else {
    HIPCHK(hipMemcpyAsync(h->pose_bak.p, h->pose.p, np, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->vel_bak.p, h->vel.p, nv, hipMemcpyDeviceToDevice, h->stream));
  }
  if (h->nl > 0) {
    const size_t nb = (size_t)h->nl * sizeof(double);
    HIPCHK(h->lmk_bak.reserve(nb));
    if (restore) HIPCHK(hipMemcpyAsync(h->lmk.p, h->lmk_bak.p, nb, hipMemcpyDeviceToDevice, h->stream));
    else HIPCHK(hipMemcpyAsync(h->lmk_bak.p, h->lmk.p, nb, hipMemcpyDeviceToDevice, h->stream));
  }
  return 0;
}

// chol_upper(Qc^-1) as the record forms read it from device memory (FusedArgs::Ud, AsmArgs::Ud): the one Qc every prior was added
// with, or the handle's.  compile() and, after a set_qc, the next launch that reads it come through here (36 doubles, stream-ordered).
int refresh_dU(gpslam_hip_handle *h) {
  if (h->dU_version == h->U_version) return 0;
  const double *U = h->gp_single_q > 0 ? &h->gp_Utab[(size_t)(h->gp_single_q - 1) * 36] : h->U;
  HIPCHK(h->dU.reserve(36 * sizeof(double)));
  HIPCHK(hipMemcpyAsync(h->dU.p, U, 36 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  h->U_diag = true;     // (6 x 6, zero below the diagonal: U is upper triangular; only the SE(3) forms ask)
  for (int i = 0; i < 6; i++)
    for (int j = i + 1; j < 6; j++) h->U_diag = h->U_diag && U[i * 6 + j] == 0.0;
  h->dU_version = h->U_version;
  return 0;
}

}  // namespace
