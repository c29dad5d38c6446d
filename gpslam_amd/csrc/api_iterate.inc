// api_iterate.inc -- the iteration driver: what turns "one Gauss-Newton / Levenberg-Marquardt iteration" into launches, collectives
// and a gpslam_hip_stats, for the three ways a chain can live on the machine (Scheme).  Included behind api_impl.inc (the launchers
// and compile()) inside namespace impl64 / impl32.  Top to bottom: guards, collectives (dist_*), the solve steps of each scheme,
// the halo update, statistics and the scalars of a Levenberg-Marquardt trial, the Gauss-Newton entry points, the one
// Levenberg-Marquardt loop, optimize, and the phase ABI of a caller-owned loop (include/gpslam_hip.h, "segment sharding").

namespace {   // (the driver's own functions; the entry points below are the ones api_decl.inc declares)

// ---------------------------------------------------------------- guards
enum class Scheme {
  LOCAL,     // the whole chain on this handle
  SHARDED,   // a segment of the chain: dense landmark border, interface records (nranks > 1 / force_sharded)
  SPLIT      // a piece of a chain split at shared cut states: fat separators (gpslam_hip_fs_set_split)
};
Scheme scheme(const gpslam_hip_handle *h) { return split_piece(h) ? Scheme::SPLIT : sharded(h) ? Scheme::SHARDED : Scheme::LOCAL; }
int dist_nranks(const gpslam_hip_handle *h) { return split_piece(h) ? h->fs.nranks : h->cfg.nranks; }

// (need_local, api_common.hpp: a compiled handle of any scheme, its device current)
int need_sharded(gpslam_hip_handle *h) {
  int rc = need_local(h);
  if (rc) return rc;
  return sharded(h) ? 0 : GPSLAM_E_INVALID;
}
// a piece of a split chain whose top block has been sized
int need_piece(gpslam_hip_handle *h, const char *what) {
  int rc = need_local(h);
  if (rc) return rc;
  if (!split_piece(h) || h->fs.nb_top <= 0) {
    const std::string m = std::string(what) + ": piece of a split chain -- gpslam_hip_fs_set_split before compile(), gpslam_hip_fs_set_top after it";
    return fail(h, GPSLAM_E_INVALID, m.c_str());
  }
  return 0;
}
// either kind of distributed handle (the steps both caller-owned Levenberg-Marquardt loops share)
int need_dist(gpslam_hip_handle *h) {
  int rc = need_local(h);
  if (rc) return rc;
  return scheme(h) != Scheme::LOCAL ? 0 : GPSLAM_E_INVALID;
}

// ---------------------------------------------------------------- collectives: the optimiser loops on a sharded handle / a split piece
// (round 5: gpslam_hip_set_collectives).  The phases are the ones a caller-owned loop uses; the collectives are the host's
// callbacks, enqueued on the handle's stream.

// refuses a handle that needs collectives and has none; a single rank gathers by copying
int dist_ready(gpslam_hip_handle *h, const char *what) {
  int rc;
  if (split_piece(h) && (rc = need_piece(h, what))) return rc;
  if (dist_nranks(h) > 1 && !h->coll_gather) {
    std::string m = std::string(what) + " on a sharded handle / split piece needs the host's collectives (gpslam_hip_set_collectives), or the caller-owned phase loop";
    return fail(h, GPSLAM_E_INVALID, m.c_str());
  }
  return 0;
}
int dist_gather(gpslam_hip_handle *h, const void *send, void *recv, size_t bytes) {
  if (dist_nranks(h) == 1 && !h->coll_gather) { HIPCHK(hipMemcpyAsync(recv, send, bytes, hipMemcpyDeviceToDevice, h->stream)); return 0; }
  if (h->coll_gather(h->coll_user, send, recv, bytes, (void *)h->stream) != 0) return fail(h, GPSLAM_E_COMM, "the all_gather callback failed");
  return 0;
}
// the ONE data-path collective of an iteration: all-gather of the interface records of either scheme
int dist_exchange(gpslam_hip_handle *h) {
  void *s = nullptr, *r = nullptr;
  size_t sb = 0, rb = 0;
  int rc;
  if (split_piece(h)) { if ((rc = IMPL_NS::gpslam_hip_fs_interface(h, &s, &sb, &r, &rb))) return rc; }
  else {
    if ((rc = IMPL_NS::gpslam_hip_interface_send(h, &s, &sb))) return rc;
    if ((rc = IMPL_NS::gpslam_hip_interface_recv(h, &r, &rb))) return rc;
  }
  return dist_gather(h, s, r, sb);
}
// dense landmark border on more than one rank: the ranks' Schur complements are summed (SURVEY 8(e) collective (3))
int dist_reduce_landmarks(gpslam_hip_handle *h) {
  if (split_piece(h) || h->nl == 0 || h->cfg.nranks <= 1) return 0;
  void *p = nullptr;
  size_t nb = 0;
  int rc = IMPL_NS::gpslam_hip_landmark_reduce_buffer(h, &p, &nb);
  if (rc) return rc;
  if (!h->coll_reduce) return fail(h, GPSLAM_E_INVALID, "a landmark border on more than one rank needs the all_reduce_sum callback");
  if (h->coll_reduce(h->coll_user, p, nb / sizeof(double), (void *)h->stream) != 0) return fail(h, GPSLAM_E_COMM, "the all_reduce_sum callback failed");
  return 0;
}
// n <= 8 scalars of every rank -> sums (mask bit clear) / maxima (bit set), in rank order: one all-gather of 64 bytes per rank.
// Every rank reduces the same gathered numbers in the same order, so all of them see bit-identical results.
int dist_scalars(gpslam_hip_handle *h, double *v, int n, unsigned max_mask) {
  const int P = dist_nranks(h);
  if (P == 1 && !h->coll_gather) return 0;
  double mine[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n; k++) mine[k] = v[k];
  HIPCHK(h->coll_s.reserve(8 * sizeof(double)));
  HIPCHK(h->coll_r.reserve((size_t)P * 8 * sizeof(double)));
  HIPCHK(hipMemcpyAsync(h->coll_s.p, mine, sizeof(mine), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));                     // (`mine` is pageable stack memory)
  int rc = dist_gather(h, h->coll_s.p, h->coll_r.p, 8 * sizeof(double));
  if (rc) return rc;
  std::vector<double> all((size_t)P * 8);
  HIPCHK(hipMemcpyAsync(all.data(), h->coll_r.p, all.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int k = 0; k < n; k++) {
    double acc = all[k];
    for (int r = 1; r < P; r++) acc = ((max_mask >> k) & 1u) ? std::fmax(acc, all[(size_t)r * 8 + k]) : acc + all[(size_t)r * 8 + k];
    v[k] = acc;
  }
  return 0;
}

// ---- Failures on ONE rank inside a collective loop (ADVICE r5).  Every rank must make the same sequence of collective calls: a rank
// that returned at its first local error would leave its peers blocked in the next all-gather.  So a local failure (a HIP error, a
// phase's status) is only RECORDED (`lrc`, the first one wins), the rank skips the local work that follows and goes on making every
// collective call of the iteration with whatever its buffers hold; the failure code then travels in a spare slot of the 64-byte
// scalar gather (maximum over the ranks of -code) and EVERY rank returns the same error.  What can still desynchronise ranks: a rank
// that never enters the call (not compiled, no collectives registered: dist_ready), a collective callback that itself fails or hangs,
// and a HIP failure inside the scalar gather's own two small copies.
struct DistErr {
  int lrc = 0;
  bool ok() const { return lrc == 0; }
  void note(int rc) { if (rc != 0 && lrc == 0) lrc = rc; }
  double slot() const { return lrc ? (double)(-lrc) : 0.0; }           // codes are negative: the slot carries a positive number
  static int decode(double v) { return v != 0.0 ? -(int)v : 0; }
};

// ---------------------------------------------------------------- the solve steps of a sharded handle (a split piece's: fs_split_phase1,
// in api_impl.inc, fs_split_solve in fatsep.hip)

// phase 1: linearise, assemble, eliminate the local segment down to its separator -> interface record.  lm_trial: the rows are those
// of the linearisation point (lm_begin) and the assembly also stores the gradient.
// clear_flag = false: inside a multi-iteration run (dist_run_gn) the non-positive-pivot flag is sticky
int sharded_phase1(gpslam_hip_handle *h, double lambda, bool lm_trial, bool clear_flag) {
  int rc;
  const LaunchMode m = lm_trial ? LaunchMode{} : level0_mode(h);
  h->ph_lambda = lambda;
  if (clear_flag) HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  if (!lm_trial && (rc = launch_factors(h, m, 0, 0))) return rc;
  if (!m.fused && (rc = launch_assemble(h, m, lm_trial))) return rc;
  return launch_forward(h, m, lambda);
}

// phase 2 (after the all-gather of the records into interface_recv): every rank solves the P-block reduced
// system redundantly and back-substitutes its segment (2a); with landmarks it then forms its share of the landmark
// Schur complement, which the caller sums over the ranks (one all-reduce of gpslam_hip_landmark_reduce_buffer);
// 2b solves the landmark system (redundantly), corrects the chain update, retracts the states, the landmarks and
// the local copy of the halo state.  st (optional) returns THIS RANK's error terms and |delta|_inf; the caller
// reduces them across ranks.
int sharded_phase2a(gpslam_hip_handle *h) {
  int rc;
  const int P = h->cfg.nranks, b = h->b, R = h->R;
  const size_t BS = (size_t)2 * b * b + (size_t)b * R;
  k_iface_build<Real><<<dim3(nblocks(P * (int)BS, 256)), dim3(256), 0, h->stream>>>(h->iface_recv.as<Real>(), P, b, R, h->top_blk.as<Real>());
  {
    FwdArgs<Real> a;
    a.blk = h->top_blk.as<Real>(); a.add = nullptr; a.up_blk = nullptr; a.up_add = nullptr;
    a.n = P; a.m = P; a.R = R; a.no_sep = 1; a.last_has_right = 0; a.remote_add = nullptr; a.lambda = Real(0);
    a.flag = h->flag.as<int>(); a.l1_blk = nullptr; a.tail = 0;
    if ((rc = launch_fwd(h, LaunchMode{}, a, 1))) return rc;
    BwdArgs<Real> bw;
    bw.blk = h->top_blk.as<Real>(); bw.x = h->top_x.as<Real>(); bw.xup = nullptr;
    bw.n = P; bw.m = P; bw.R = R; bw.no_sep = 1; bw.last_has_right = 0;
    launch_bwd(h, bw, 1);
  }
  const Real *xtop = h->top_x.as<Real>() + (size_t)h->cfg.rank * b * R;   // [x_sep(rank), x_sep(rank + 1)]
  if ((rc = launch_backward(h, xtop))) return rc;
  // the ranks' Schur complements are summed: the LM damping of the landmark block goes in exactly once
  return launch_landmarks_reduce(h, (h->cfg.nranks > 1 && h->cfg.rank != 0) ? 0.0 : h->ph_lambda);
}

// ---- the halo state: the local copy of the right neighbour's first state, kept in step with its owner.  Its update is the reduced
// solve's x_sep(rank + 1) ...
Real *halo_x(gpslam_hip_handle *h) { return h->top_x.as<Real>() + ((size_t)h->cfg.rank + 1) * h->b * h->R; }
// ... which needs the landmark correction too: delta = x0 - Z dL on that one block
void correct_halo(gpslam_hip_handle *h) {
  if (h->nl == 0) return;
  LmArgs<Real, RowT> la = lm_args(h, 0.0);
  la.N = 1; la.x = halo_x(h);
  k_lm_correct<Real, RowT><<<dim3(nblocks(h->b, 256)), dim3(256), 0, h->stream>>>(la);
}
void retract_halo(gpslam_hip_handle *h) {
  RetractArgs<Real> a;
  a.pose = h->pose.as<double>(); a.vel = h->vel.as<double>(); a.stride = h->stride; a.N = 1; a.R = h->R;
  a.chart = h->cfg.chart; a.first = h->N; a.x = halo_x(h); a.partial = h->partial.as<Real>() + nblocks(h->N, 128) + 4; a.flag = h->flag.as<int>();
  dispatch_mf(h->mf, [&](auto tag) {
    constexpr int MF = decltype(tag)::value;
    k_retract<Real, MF><<<dim3(1), dim3(128), 0, h->stream>>>(a);
  });
}

// ---------------------------------------------------------------- statistics
void set_stats(gpslam_hip_stats *st, double before, double after, double dinf, int iters, int accepted, int status) {
  if (!st) return;
  std::memset(st, 0, sizeof(*st));
  st->error_before = before; st->error_after = after; st->delta_inf_norm = dinf;
  st->iterations = iters; st->accepted = accepted; st->status = status;
}
// what the device left of the last of `iters` Gauss-Newton iterations on this handle: scal[0..2] and the pivot flag -> st (optional).
// A non-positive pivot is st->status and the return code; any other code is the read's own failure (st untouched).
int gn_stats(gpslam_hip_handle *h, int iters, gpslam_hip_stats *st) {
  double s[4];
  int flag = 0;
  int rc = read_scal(h, s, 4, &flag);
  if (rc) return rc;
  set_stats(st, s[0], s[1], s[2], iters, 1, flag ? GPSLAM_E_NOT_SPD : 0);
  return flag ? fail(h, GPSLAM_E_NOT_SPD, "non-positive pivot in the block elimination") : 0;
}
// one Levenberg-Marquardt iteration, from the numbers of its last trial (o = out6 of trial_scalars, summed over the ranks)
void lm_stats(gpslam_hip_stats *st, const double *o, bool accepted, double lambda, int trials) {
  set_stats(st, o[0], accepted ? o[1] : o[0], accepted ? o[2] : 0.0, 1, accepted ? 1 : 0, 0);
  if (!st) return;
  st->lambda = lambda;
  st->trials = trials;
  st->last_trial_error = o[5] == 0.0 ? o[1] : o[0];
}

// ---------------------------------------------------------------- the scalars of a Levenberg-Marquardt trial
// The trial's solve has left delta in lv[0].x (and lm_dL).  out6 = {error at the linearisation point, trial error, |delta|_inf,
// delta . g, |delta|^2, indefinite-pivot flag}, all for THIS handle's share of the chain; sums / maxima over the ranks give the
// global values.  Applies the trial update (retract) and evaluates the trial error.  What a scheme's share is:
//   local    delta . g against gsave (slot 3) and, on the fused level-0 path (m.fused), its separator parts in gsave2 (slot 8)
//   sharded  the replicated landmark update is counted once, on rank 0; the rows of the last local state also feed the gradient of
//            the neighbour's first state (halo_add = [RD | Rg]): that share of delta . g is only known here (slot 7)
//   split    delta . g adds up over the pieces as it is (every piece holds its own share of a shared unknown's gradient);
//            |delta|^2 counts a shared unknown on the piece to its right only: own states (nx_own), own landmarks (d_lm_own)
// linErr(0) - linErr(delta) = 0.5 delta.g + 0.5 lambda |delta|^2 because (H + lambda I) delta = g.
int trial_scalars(gpslam_hip_handle *h, const LaunchMode &m, double *out6) {
  int rc;
  const Scheme sc = scheme(h);
  const bool halo = has_right_rank(h);
  const bool cut_right = sc == Scheme::SPLIT && h->fs.rank < h->fs.nranks - 1;
  const bool lm_here = h->nl > 0 && (sc != Scheme::SHARDED || h->cfg.rank == 0);
  const int b = h->b, nl = h->nl, nx = h->N * b, nx_own = (h->N - (cut_right ? 1 : 0)) * b;
  Real *dv = h->dvec.as<Real>(), *dL = h->lm_dL.as<Real>();
  if (halo) correct_halo(h);
  k_gather_delta<Real><<<dim3(nblocks(nx, 256)), dim3(256), 0, h->stream>>>(h->lv[0].x.as<Real>(), h->N, h->R, b, dv);
  if (sc == Scheme::LOCAL) {      // delta . g (slot 3), its separator parts (fused: slot 8), |delta|^2 (slot 4)
    if ((rc = launch_dot3(h, dv, h->gsave.as<Real>(), m.fused ? h->gsave2.as<Real>() : nullptr, nx, 3, 8, 4))) return rc;
  } else {
    if ((rc = launch_dot(h, dv, h->gsave.as<Real>(), nx, 3))) return rc;
    if ((rc = launch_dot(h, dv, dv, nx_own, 4))) return rc;
  }
  if (lm_here) {
    const Real *gL = h->fs.active ? h->lm_gL.as<Real>() : h->lm_S.as<Real>() + (size_t)nl * h->R, *own = dL;
    if ((rc = launch_dot(h, dL, gL, nl, 5))) return rc;
    if (sc == Scheme::SPLIT) {
      fs_mask_mul(h, dL, h->stream);
      own = h->fs.lm_tmp.as<Real>();
    }
    if ((rc = launch_dot(h, own, dL, nl, 6))) return rc;
  }
  if (halo && (rc = launch_dot(h, halo_x(h), h->halo_add.as<Real>() + (size_t)b * b, b, 7))) return rc;
  if ((rc = launch_retract(h, m, 2))) return rc;
  if (halo) retract_halo(h);
  if ((rc = launch_factors(h, LaunchMode{}, 1, 1))) return rc;   // scal[1] = trial error
  double s[10];
  int flag = 0;
  if ((rc = read_scal(h, s, 10, &flag))) return rc;
  out6[0] = s[0]; out6[1] = s[1]; out6[2] = s[2];
  out6[3] = s[3] + (m.fused ? s[8] : 0.0) + (halo ? s[7] : 0.0) + (lm_here ? s[5] : 0.0);
  out6[4] = s[4] + (lm_here ? s[6] : 0.0);
  out6[5] = flag ? 1.0 : 0.0;
  return 0;
}

// ---------------------------------------------------------------- Gauss-Newton
// 2b of a sharded iteration: landmark solve, update of the states and of the halo state
int sharded_phase2b(gpslam_hip_handle *h, gpslam_hip_stats *st) {
  int rc;
  if ((rc = launch_landmarks_solve(h, h->ph_lambda))) return rc;
  if ((rc = launch_retract(h, LaunchMode{}, 2))) return rc;
  if (has_right_rank(h)) { correct_halo(h); retract_halo(h); }
  // the error of the new state: only when the caller wants statistics (inside a fixed-count run the next
  // iteration's linearisation evaluates it anyway)
  if (st && (rc = launch_factors(h, LaunchMode{}, 1, 1))) return rc;
  HIPCHK(hipGetLastError());
  return st ? gn_stats(h, 1, st) : 0;
}
int fs_split_phase2(gpslam_hip_handle *h, gpslam_hip_stats *st) {
  int rc;
  if ((rc = fs_split_solve(h))) return rc;
  if ((rc = launch_retract(h, LaunchMode{}, 2))) return rc;
  if (st && (rc = launch_factors(h, LaunchMode{}, 1, 1))) return rc;
  HIPCHK(hipGetLastError());
  return st ? gn_stats(h, 1, st) : 0;
}

// one Gauss-Newton iteration over all ranks / pieces.  loc (optional): THIS rank's statistics.  Returns only what a collective itself
// reported (then the ranks are out of step anyway); local failures go to `de`.
int dist_gn_step(gpslam_hip_handle *h, gpslam_hip_stats *loc, DistErr &de) {
  int rc;
  const bool split = split_piece(h);
  if (de.ok()) de.note(split ? fs_split_phase1(h, 0.0, false, false) : sharded_phase1(h, 0.0, false, false));
  if ((rc = dist_exchange(h))) return rc;
  if (!split) {
    if (de.ok()) de.note(sharded_phase2a(h));
    if ((rc = dist_reduce_landmarks(h))) {
      if (rc != GPSLAM_E_COMM) return rc;
      de.note(rc);                                      // this rank's callback failed: tell the others through the scalars
    }
  }
  if (de.ok()) {
    rc = split ? fs_split_phase2(h, loc) : sharded_phase2b(h, loc);
    if (rc != GPSLAM_E_NOT_SPD) de.note(rc);            // (a non-positive pivot is a property of the graph, reduced with the statistics)
    else if (loc) loc->status = GPSLAM_E_NOT_SPD;
  }
  return 0;
}
// GaussNewtonOptimizer::iterate (iters = 1) / gpslam_hip_run_gn over all ranks / pieces: `iters` iterations, st (optional) the
// statistics of the last one over the whole chain.  The non-positive-pivot flag is cleared ONCE and stays up through the run (phase 1
// does not clear it), a local failure of any iteration is carried to the ONE scalar gather at the end -- which runs with or without
// st: it is also how a rank learns that another one failed.  An indefinite pivot or an error in iteration k < last is reported by
// every rank with the same code, as the unsharded run_gn reports it (ADVICE r5: both used to be swallowed).
int dist_run_gn(gpslam_hip_handle *h, const char *what, int iters, gpslam_hip_stats *st) {
  int rc = dist_ready(h, what);
  if (rc) return rc;
  gpslam_hip_stats loc;
  std::memset(&loc, 0, sizeof(loc));
  DistErr de;
  de.note(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream) == hipSuccess ? 0 : GPSLAM_E_HIP);
  for (int it = 0; it < iters; it++)
    if ((rc = dist_gn_step(h, (it == iters - 1) ? &loc : nullptr, de))) return rc;
  double v[5] = {loc.error_before, loc.error_after, loc.delta_inf_norm, loc.status == GPSLAM_E_NOT_SPD ? 1.0 : 0.0, de.slot()};
  if ((rc = dist_scalars(h, v, 5, 0x1Cu))) return rc;   // sums of [0], [1]; maxima of [2], [3], [4]
  set_stats(st, v[0], v[1], v[2], iters, 1, v[4] != 0.0 ? DistErr::decode(v[4]) : (v[3] != 0.0 ? GPSLAM_E_NOT_SPD : 0));
  if (v[4] != 0.0) return fail(h, DistErr::decode(v[4]), de.ok() ? "another rank failed inside the iteration" : "this rank failed inside the iteration (every rank returns its code)");
  if (v[3] != 0.0) return fail(h, GPSLAM_E_NOT_SPD, "non-positive pivot in the block elimination (on some rank)");
  return 0;
}

}  // namespace

int gpslam_hip_iterate_gn(gpslam_hip_handle *h, gpslam_hip_stats *st) {
  int rc = need_local(h);
  if (rc) return rc;
  if (scheme(h) != Scheme::LOCAL) return dist_run_gn(h, "iterate_gn", 1, st);   // (refuses without the host's collectives: the phase loop is the caller's then)
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  const LaunchMode m = gn_mode(h, true, true);
  if ((rc = enqueue_gn(h, m, 0.0, true, true, false))) return rc;
  gpslam_hip_stats loc;
  const int pivot = gn_stats(h, 1, &loc);
  if (pivot && pivot != GPSLAM_E_NOT_SPD) return pivot;
  for (int i = 0; i < 5; i++) h->last_ms[i] = 0;
  h->l0_ms = 0.0;
  if ((rc = collect_timing(h, m, h->last_ms))) return rc;
  if (st) *st = loc;
  if (pivot) return pivot;
  if (!(loc.error_after == loc.error_after)) return fail(h, GPSLAM_E_NAN, "NaN error after update");
  return 0;
}

int gpslam_hip_run_gn(gpslam_hip_handle *h, int32_t iters, gpslam_hip_stats *st, double *out5) {
  int rc = need_local(h);
  if (rc) return rc;
  if (iters <= 0) return GPSLAM_E_INVALID;
  if (scheme(h) != Scheme::LOCAL) {   // all ranks / pieces: ONE small all-gather at the end (statistics of the last iteration + failures of any)
    if (out5) for (int i = 0; i < 5; i++) out5[i] = 0.0;
    return dist_run_gn(h, "run_gn", iters, st);
  }
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  double acc[5] = {0, 0, 0, 0, 0};
  h->l0_ms = 0.0;
  // never leave an update unapplied behind an error (ADVICE r5: EVERY exit, not only enqueue_gn's): the accessors of the states
  // (get_states, set_halo, the next linearisation) read h->pose / h->vel as they are
  auto bail = [&](int code) {
    if (h->defer.update) { (void)flush_update(h); (void)hipStreamSynchronize(h->stream); }
    return code;
  };
  for (int it = 0; it < iters; it++) {
    const bool timed = (out5 != nullptr);
    const bool last = it == iters - 1;
    // (round 5) every iteration but the last leaves its retraction to the next iteration's K1 (PendUpd); |delta|_inf and the error
    // are reported for the last iteration, as before
    const LaunchMode m = gn_mode(h, timed, last);
    if ((rc = enqueue_gn(h, m, 0.0, timed, last, h->plan.fold_retract && !last))) return bail(rc);
    if (timed) {
      if (hipEventSynchronize(h->ev[4]) != hipSuccess) { h->err = "hipEventSynchronize failed inside run_gn"; return bail(GPSLAM_E_HIP); }
      if ((rc = collect_timing(h, m, acc))) return bail(rc);
    }
  }
  rc = gn_stats(h, iters, st);
  if (rc && rc != GPSLAM_E_NOT_SPD) return bail(rc);
  if (out5) for (int i = 0; i < 5; i++) out5[i] = acc[i];
  return rc;
}

// ---------------------------------------------------------------- Levenberg-Marquardt
namespace {
// linearise once at the current estimate (rows + scal[0] = this handle's error) and remember it
int lm_begin(gpslam_hip_handle *h, const LaunchMode &m) {
  int rc;
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  if ((rc = launch_factors(h, m, 0, 0))) return rc;
  return backup_state(h, false);
}
// a local trial's solve at lambda; the rows are still those of the linearisation point
int local_lm_solve(gpslam_hip_handle *h, const LaunchMode &m, double lambda) {
  int rc;
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  if (!m.fused && (rc = launch_assemble(h, m, true))) return rc;
  return launch_solve(h, m, lambda);
}

}  // namespace

// LevenbergMarquardtOptimizer::iterate (GTSAM 4.0 defaults: diagonalDamping = false, fixed lambda factor):
// linearise once; tryLambda { damp with lambda I; solve; rho = (err - newErr) / (linErr(0) - linErr(delta));
// keep the step if rho > minModelFidelity and lambda /= factor; otherwise, if |err - newErr| < relativeErrorTol * err,
// stop with lambda and the values untouched; otherwise lambda *= factor and again, giving up at lambdaUpperBound }.
// ONE loop for the three schemes.  On a sharded handle / split piece the trial's scalars are summed over the ranks, so every
// branch is gpslam_hip_lm_decide on identical numbers, and local failures follow DistErr (slot 6 of the gather).  A local handle
// makes no collective calls: a failure ends the call at the next `local failure` line, nothing having been launched behind it.
int gpslam_hip_iterate_lm(gpslam_hip_handle *h, double *lambda, const gpslam_hip_params *p, gpslam_hip_stats *st) {
  int rc = need_local(h);
  if (rc) return rc;
  if (!lambda || !p) return GPSLAM_E_INVALID;
  const Scheme sc = scheme(h);
  const bool dist = sc != Scheme::LOCAL;
  if (dist && (rc = dist_ready(h, "iterate_lm"))) return rc;   // (refuses without the host's collectives)
  // local Pose3-sized chains without landmarks: every trial is the fused level-0 kernel (it re-assembles from the row tables /
  // structured records of the linearisation point with the trial's lambda, and leaves the gradient in gsave / gsave2)
  LaunchMode m;
  if (!dist) { m = level0_mode(h); m.gsave = m.fused; }
  DistErr de;
  de.note(lm_begin(h, m));
  bool accepted = false;
  double o[7];
  int trials = 0;
  for (;;) {
    for (double &x : o) x = 0.0;
    switch (sc) {                                           // solve at lambda
      case Scheme::LOCAL:
        if (de.ok()) de.note(local_lm_solve(h, m, *lambda));
        break;
      case Scheme::SHARDED:
        if (de.ok()) de.note(sharded_phase1(h, *lambda, true, true));
        if ((rc = dist_exchange(h))) return rc;
        if (de.ok()) de.note(sharded_phase2a(h));
        if ((rc = dist_reduce_landmarks(h))) {
          if (rc != GPSLAM_E_COMM) return rc;
          de.note(rc);
        }
        if (de.ok()) de.note(launch_landmarks_solve(h, h->ph_lambda));
        break;
      case Scheme::SPLIT:
        if (de.ok()) de.note(fs_split_phase1(h, *lambda, true, true));
        if ((rc = dist_exchange(h))) return rc;
        if (de.ok()) de.note(fs_split_solve(h));
        break;
    }
    if (de.ok()) de.note(trial_scalars(h, m, o));
    if (!dist && !de.ok()) return de.lrc;                   // local failure
    o[6] = de.slot();
    if (dist && (rc = dist_scalars(h, o, 7, 0x64u))) return rc;   // sums of [0], [1], [3], [4]; maxima of [2], [5], [6]
    if (o[6] != 0.0) {                                      // some rank failed: every rank leaves the loop here, with its code
      if (de.ok()) (void)backup_state(h, true);             // (this rank's trial update is not kept)
      return fail(h, DistErr::decode(o[6]), de.ok() ? "another rank failed inside the Levenberg-Marquardt trial" : "this rank failed inside the Levenberg-Marquardt trial");
    }
    trials++;
    int32_t ok = 0, done = 0;
    if ((rc = ::gpslam_hip_lm_decide(o, p, lambda, &ok, &done))) return rc;     // (host arithmetic on identical numbers: the same on every rank)
    if (ok) { accepted = true; break; }
    de.note(backup_state(h, true));                         // not kept: restore the linearisation point (a failure here is reported by the next trial's gather, or below)
    if (!dist && !de.ok()) return de.lrc;                   // local failure
    if (done) break;                                        // small cost change (lambda untouched) or lambda at its bound
  }
  if (!de.ok()) {                                           // a reject that failed behind the last trial: one more 64-byte round so that all ranks agree
    double v[1] = {de.slot()};
    if ((rc = dist_scalars(h, v, 1, 0x1u))) return rc;
    return fail(h, DistErr::decode(v[0]), "restoring the linearisation point failed on some rank");
  } else if (dist && !accepted) {                           // (the same round on the ranks whose reject went through)
    double v[1] = {0.0};
    if ((rc = dist_scalars(h, v, 1, 0x1u))) return rc;
    if (v[0] != 0.0) return fail(h, DistErr::decode(v[0]), "restoring the linearisation point failed on another rank");
  }
  lm_stats(st, o, accepted, *lambda, trials);
  return 0;
}

int gpslam_hip_error(gpslam_hip_handle *h, double *err) {
  int rc = need_local(h);
  if (rc) return rc;
  if (!err) return GPSLAM_E_INVALID;
  double s[4] = {0, 0, 0, 0};
  int flag;
  rc = launch_factors(h, LaunchMode{}, 1, 1);
  if (!rc) rc = read_scal(h, s, 4, &flag);
  *err = s[1];
  // (with the host's collectives registered: the error of the whole chain, NonlinearFactorGraph::error -- a collective call, which a
  //  rank whose own evaluation failed still takes part in: the failure code rides beside the sum and every rank returns it)
  if (scheme(h) != Scheme::LOCAL && h->coll_gather) {
    double v[2] = {s[1], rc ? (double)(-rc) : 0.0};
    int rc2 = dist_scalars(h, v, 2, 0x2u);
    if (rc2) return rc2;
    *err = v[0];
    if (v[1] != 0.0) return fail(h, -(int)v[1], rc ? "evaluating the error failed on this rank" : "evaluating the error failed on another rank");
    return 0;
  }
  return rc;
}

int gpslam_hip_optimize(gpslam_hip_handle *h, const gpslam_hip_params *p, gpslam_hip_stats *st) {
  int rc = need_compiled(h);
  if (rc) return rc;
  if (!p) return GPSLAM_E_INVALID;
  // NonlinearOptimizer::defaultOptimize: do { cur = error(); iterate(); } while (!converged)
  double err0;
  if ((rc = IMPL_NS::gpslam_hip_error(h, &err0))) return rc;
  gpslam_hip_stats it;
  std::memset(&it, 0, sizeof(it));
  double new_err = err0, dinf = 0.0, lambda = p->lambda_initial;
  int iters = 0;
  if (!(err0 <= p->error_tol)) {
    for (;;) {
      const double cur = new_err;
      rc = p->use_lm ? IMPL_NS::gpslam_hip_iterate_lm(h, &lambda, p, &it) : IMPL_NS::gpslam_hip_iterate_gn(h, &it);
      if (rc) break;
      iters++;
      new_err = it.error_after;
      dinf = it.delta_inf_norm;
      if (iters >= p->max_iterations) break;
      if (new_err <= p->error_tol) break;
      const double abs_dec = cur - new_err, rel_dec = abs_dec / cur;
      if (rel_dec <= p->relative_error_tol || abs_dec <= p->absolute_error_tol) break;
      if (p->delta_tol > 0.0 && dinf < p->delta_tol) break;
      if (p->use_lm && !it.accepted) break;
    }
  }
  set_stats(st, err0, new_err, dinf, iters, 1, rc);
  if (st) st->lambda = lambda;
  return rc;
}

// ---------------------------------------------------------------- the phase ABI: segment sharding
// A caller-owned loop (gpslam_amd/sharded.py, gpslam_amd/host/sharded_host.hpp) drives the same pieces and makes the collectives
// itself.  Gauss-Newton: iterate_phase1 -> all-gather of the interface records -> phase2a -> all-reduce of the landmark buffer
// -> phase2b.  Levenberg-Marquardt needs three global sums per trial (error, delta . g, |delta|^2):
//   lm_begin            linearise once at the current estimate, remember it
//   lm_trial_phase1     damp with lambda, eliminate the segment            -> all-gather of the interface records
//   iterate_phase2a     reduced solve, back-substitution, landmark share   -> all-reduce of the landmark buffer
//   lm_trial_phase2     landmark solve, trial update, this rank's scalars  -> all-reduce of the scalars, decision
//   lm_reject           back to the linearisation point (an accepted trial needs nothing)
int gpslam_hip_interface_send(gpslam_hip_handle *h, void **dev_ptr, size_t *bytes) {
  int rc = need_sharded(h);
  if (rc) return rc;
  if (!dev_ptr || !bytes) return GPSLAM_E_INVALID;
  const size_t BS = (size_t)2 * h->b * h->b + (size_t)h->b * h->R, AS = (size_t)h->b * h->b + (size_t)h->b * h->R;
  *dev_ptr = h->iface_send.p;
  *bytes = (BS + AS) * sizeof(Real);
  return 0;
}
int gpslam_hip_interface_recv(gpslam_hip_handle *h, void **dev_ptr, size_t *bytes) {
  int rc = IMPL_NS::gpslam_hip_interface_send(h, dev_ptr, bytes);   // (the size of one rank's record)
  if (rc) return rc;
  *dev_ptr = h->iface_recv.p;
  *bytes *= (size_t)h->cfg.nranks;
  return 0;
}
int gpslam_hip_landmark_reduce_buffer(gpslam_hip_handle *h, void **dev_ptr, size_t *bytes) {
  if (!h || !dev_ptr || !bytes) return GPSLAM_E_INVALID;
  *dev_ptr = h->nl > 0 ? h->lm_S.p : nullptr;
  *bytes = h->nl > 0 ? ((size_t)h->nl * h->R + h->nl) * sizeof(Real) : 0;
  return 0;
}
int gpslam_hip_iterate_phase1(gpslam_hip_handle *h, double lambda) {
  int rc = need_sharded(h);
  return rc ? rc : sharded_phase1(h, lambda, false, true);
}
int gpslam_hip_iterate_phase2a(gpslam_hip_handle *h) {
  int rc = need_sharded(h);
  return rc ? rc : sharded_phase2a(h);
}
int gpslam_hip_iterate_phase2b(gpslam_hip_handle *h, gpslam_hip_stats *st) {
  int rc = need_sharded(h);
  return rc ? rc : sharded_phase2b(h, st);
}
// 2a + 2b for chains without landmarks (or a single rank): nothing to reduce in between
int gpslam_hip_iterate_phase2(gpslam_hip_handle *h, gpslam_hip_stats *st) {
  if (h && h->nl > 0 && h->cfg.nranks > 1)
    return fail(h, GPSLAM_E_INVALID, "landmarks on a sharded chain: phase2a, all-reduce of the landmark buffer, phase2b");
  int rc = IMPL_NS::gpslam_hip_iterate_phase2a(h);
  return rc ? rc : IMPL_NS::gpslam_hip_iterate_phase2b(h, st);
}
int gpslam_hip_lm_begin(gpslam_hip_handle *h) {
  int rc = need_dist(h);
  return rc ? rc : lm_begin(h, LaunchMode{});
}
int gpslam_hip_lm_trial_phase1(gpslam_hip_handle *h, double lambda) {
  int rc = need_sharded(h);
  return rc ? rc : sharded_phase1(h, lambda, true, true);
}
int gpslam_hip_lm_trial_phase2(gpslam_hip_handle *h, double *out6) {
  int rc = need_sharded(h);
  if (rc) return rc;
  if (!out6) return GPSLAM_E_INVALID;
  if ((rc = launch_landmarks_solve(h, h->ph_lambda))) return rc;
  return trial_scalars(h, LaunchMode{}, out6);
}
int gpslam_hip_lm_reject(gpslam_hip_handle *h) {
  int rc = need_dist(h);
  return rc ? rc : backup_state(h, true);
}

// ---------------------------------------------------------------- the phase ABI: a chain split into pieces
// config 4 across GPUs: the segmented landmark elimination on a chain split into pieces (DESIGN.md section 5).
// compile() has planned this piece with its end blocks kept (FatSepPlan::split); set_top sizes the interface record once
// the caller knows the widest fat block of any piece.  Gauss-Newton: fs_phase1 -> all-gather of the records -> fs_phase2.
// Levenberg-Marquardt (the caller's loop, as for the dense-border sharding above): gpslam_hip_lm_begin; per trial
// fs_lm_trial_phase1(lambda) -> all-gather of the records -> fs_lm_trial_phase2(out6) -> all-reduce of out6 -> accept, or
// gpslam_hip_lm_reject and a larger lambda.  (gpslam_hip_fs_split_info and gpslam_hip_fs_set_top: fatsep.hip.)
int gpslam_hip_fs_interface(gpslam_hip_handle *h, void **send, size_t *send_bytes, void **recv, size_t *recv_bytes) {
  int rc = need_piece(h, "fs_interface");
  if (rc) return rc;
  if (!send || !send_bytes || !recv || !recv_bytes) return GPSLAM_E_INVALID;
  FatSepPlan &p = h->fs;
  const size_t RS = ((size_t)3 * p.nb_top * p.nb_top + 2 * p.nb_top) * sizeof(Real);
  *send = p.send.p; *send_bytes = RS;
  *recv = p.recv.p; *recv_bytes = (size_t)p.nranks * RS;
  return 0;
}
int gpslam_hip_fs_phase1(gpslam_hip_handle *h, double lambda) {
  int rc = need_piece(h, "fs_phase1");
  return rc ? rc : fs_split_phase1(h, lambda, false, true);
}
int gpslam_hip_fs_phase2(gpslam_hip_handle *h, gpslam_hip_stats *st) {
  int rc = need_piece(h, "fs_phase2");
  return rc ? rc : fs_split_phase2(h, st);
}
int gpslam_hip_fs_lm_trial_phase1(gpslam_hip_handle *h, double lambda) {
  int rc = need_piece(h, "fs_lm_trial_phase1");
  return rc ? rc : fs_split_phase1(h, lambda, true, true);
}
int gpslam_hip_fs_lm_trial_phase2(gpslam_hip_handle *h, double *out6) {
  int rc = need_piece(h, "fs_lm_trial_phase2");
  if (rc) return rc;
  if (!out6) return GPSLAM_E_INVALID;
  if ((rc = fs_split_solve(h))) return rc;
  return trial_scalars(h, LaunchMode{}, out6);
}
