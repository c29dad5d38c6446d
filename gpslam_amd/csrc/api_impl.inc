// api_impl.inc -- the precision-dependent half of libgpslam_hip.so's host side: argument packing and launches, compile(), the
// inspection calls.  The iteration driver follows it in api_iterate.inc.  Both are included twice, by api_impl64.hip inside
// namespace impl64 (RowT = double: GPSLAM_FP64) and by api_impl32.hip inside namespace impl32 (RowT = float: GPSLAM_FP32); the
// extern "C" entry points in api.hip dispatch on the handle's precision (GPS_BY_PRECISION).  RowT is the type the factor kernels compute the Jacobians in
// and of the row tables in HBM (the dominant traffic of an iteration); Real -- the normal equations and the solver -- is
// double in both: J^T J squares the condition number, and a 1e5-state chain anchored by one prior (BASELINE config 3) is
// beyond what an fp32 factorisation survives (measured: non-positive pivots).  States, landmarks and factor parameters
// are fp64 as well (kernels.hpp, GpArgs), and an fp32 handle's residual is evaluated by the fp64 error pass.
constexpr bool kIsF64 = std::is_same<RowT, double>::value;   // RowT: Jacobian row tables; Real (solver) is double in both
UMat<RowT> make_umat(const gpslam_hip_handle *h) {
  UMat<RowT> u;
  for (int i = 0; i < 36; i++) u.u[i] = 0;
  for (int i = 0; i < h->d * h->d; i++) u.u[i] = (RowT)h->U[i];
  return u;
}

// grp < 0: every GP prior in one launch (they share the handle's Qc); grp >= 0: the factors of Qc group grp -- the
// device-side factor arrays are ordered by Qc when a graph has more than one (compile(), gpslam_hip_add_gp_priors_qc)
GpArgs<RowT> gp_args(gpslam_hip_handle *h, const LaunchMode &m, RowT *partial, bool e32 = false, int grp = -1) {
  GpArgs<RowT> a;
  a.pose = h->pose.as<double>(); a.vel = h->vel.as<double>(); a.stride = h->stride;
  a.count = (int)h->gp_left.size();
  a.left = h->d_gp_left.as<int>(); a.dt = h->d_gp_dt.as<double>(); a.row0 = h->d_gp_row0.as<int>();
  a.rowLR = h->rowLR.as<RowT>(); a.rowE = h->rowE.as<RowT>(); a.rowE32 = e32 ? h->rowE.as<float>() : nullptr;
  a.partial = partial; a.out_e = nullptr; a.out_H = nullptr;
  a.U = make_umat(h);
  if (grp >= 0) {
    const int q = h->gp_groups[3 * grp], first = h->gp_groups[3 * grp + 1];
    a.count = h->gp_groups[3 * grp + 2];
    a.left += first; a.dt += first; a.row0 += first;
    if (q > 0) {
      for (int i = 0; i < 36; i++) a.U.u[i] = 0;
      for (int i = 0; i < h->d * h->d; i++) a.U.u[i] = (RowT)h->gp_Utab[(size_t)(q - 1) * 36 + i];
    }
  }
  a.vw = h->vw;
  a.gps = gp_form(h, m) != GpForm::Rows ? h->gps.as<RowT>() : nullptr;
  return a;
}
int gp_ngroups(const gpslam_hip_handle *h) { return (int)h->gp_groups.size() / 3; }
// K1 of the GP priors alone (several Qc groups; gpslam_hip_time_kernel): rows, or structured records where a.gps says so
template <int MF> void launch_gp_rows(gpslam_hip_handle *h, const GpArgs<RowT> &a, int nb) {
  if constexpr ((MF == POSE3 || MF == POSE2 || MF == ROT3 || MF == LINEAR3) && kIsF64) {
    if (a.gps != nullptr) { k_gp<RowT, MF, 0, false, true><<<dim3(nb), dim3(128), 0, h->stream>>>(a); return; }
  }
  if (MF == POSE3 && h->vw) k_gp<RowT, MF, 0, true><<<dim3(nb), dim3(128), 0, h->stream>>>(a);
  else k_gp<RowT, MF, 0><<<dim3(nb), dim3(128), 0, h->stream>>>(a);
}

LmArgs<Real, RowT> lm_args(gpslam_hip_handle *h, double lambda) {
  LmArgs<Real, RowT> a;
  a.N = h->N; a.R = h->R; a.B = h->b; a.L = h->L; a.ld = h->ld; a.nl = h->nl;
  a.Nx = h->N + (has_right_rank(h) ? 1 : 0);
  a.rowLR = h->rowLR.as<RowT>(); a.rowE = h->rowE.as<RowT>(); a.rowM = h->rowM.as<RowT>();
  a.lmrow = h->lmrow.as<int>(); a.lmrow_state = h->lmrow_state.as<int>(); a.lmrow_ptr = h->lmrow_ptr.as<int>();
  a.nlmrows = h->nlmrows;
  a.chunk_lm = h->lm_chunk_lm.as<int>(); a.chunk_j0 = h->lm_chunk_j0.as<int>(); a.chunk_j1 = h->lm_chunk_j1.as<int>();
  a.chunk_ptr = h->lm_chunk_ptr.as<int>(); a.nchunks = h->nlmchunks; a.part = h->lm_part.as<Real>();
  a.x = h->lv.empty() ? nullptr : h->lv[0].x.as<Real>();
  a.t = h->lm_t.as<Real>();
  a.npri = h->lpri.count(); a.pri_lm = h->lpri.d_idx.as<int>(); a.pri_meas = h->lpri.d_meas.as<double>();
  a.pri_sig = h->lpri.d_sig.as<double>();
  a.lmk = h->lmk.as<double>(); a.S = h->lm_S.as<Real>(); a.gL = h->lm_S.as<Real>() + (size_t)h->nl * h->R; a.dL = h->lm_dL.as<Real>();
  a.lambda = (Real)lambda; a.flag = h->flag.as<int>(); a.partial = nullptr;
  return a;
}

// pose priors (0), velocity priors (1), between factors (2): k_lin's three sets, and the order of their partial sums
SimpleSet &simple_set(gpslam_hip_handle *h, int kind) { return kind == 0 ? h->pri : (kind == 1 ? h->vpri : h->btw); }
FacArgs<RowT> fac_args(gpslam_hip_handle *h, const LaunchForm &form, int kind, RowT *partial, bool e32) {
  SimpleSet &s = simple_set(h, kind);
  FacArgs<RowT> a;
  a.pose = h->pose.as<double>(); a.vel = h->vel.as<double>(); a.stride = h->stride;
  a.count = s.count(); a.chart = h->cfg.chart;
  a.idx = s.d_idx.as<int>(); a.meas = s.d_meas.as<double>(); a.sig = s.d_sig.as<double>(); a.row0 = s.d_row0.as<int>();
  const bool compact = (kind != 1);   // pose priors and between factors: velocity-free rows
  a.rowLR = compact ? h->rowC.as<RowT>() : h->rowLR.as<RowT>(); a.rowE = compact ? h->rowCE.as<RowT>() : h->rowE.as<RowT>();
  a.partial = partial; a.rowE32 = e32 ? (compact ? h->rowCE.as<float>() : h->rowE.as<float>()) : nullptr;
  // BetweenFactor<Pose3> of a launch whose consumer is the structured fused kernel: records instead of compact rows
  a.rec = (kind == 2 && form.btw_rec) ? h->brec.as<RowT>() : nullptr;
  return a;
}

// The factors of one measurement kind, writing nowhere yet: the caller sets the row tables or out_e / out_J, partial, and what its
// launch adds (rob, gps, pend)
MeasArgs<RowT> meas_args(gpslam_hip_handle *h, int fk) {
  MeasSet &s = h->ms[fk];
  MeasArgs<RowT> a;
  a.pose = h->pose.as<double>(); a.vel = h->vel.as<double>(); a.stride = h->stride;
  a.lmk = h->lmk.as<double>(); a.ld = h->ld; a.count = s.count(); a.chart = h->cfg.chart;
  a.idx = s.d_idx.as<int>(); a.lm = s.d_lm.as<int>(); a.meas = s.d_meas.as<double>(); a.mw = s.mw;
  a.sig = s.d_sig.as<double>(); a.coef = s.d_coef.as<double>();
  a.aux = s.any_aux ? s.d_aux.as<double>() : nullptr; a.aidx = s.any_aux ? s.d_aidx.as<int>() : nullptr;
  a.sqi = s.sqi.empty() ? nullptr : s.d_sqi.as<double>();
  a.vw = h->vw; a.row0 = s.d_row0.as<int>();
  a.rowLR = nullptr; a.rowE = nullptr; a.rowM = nullptr; a.rowLm = nullptr;
  a.partial = nullptr; a.rowE32 = nullptr; a.out_e = nullptr; a.out_J = nullptr;
  return a;
}

// A pending update (Deferred::update) applied by the separate retraction; |delta|_inf into scal[2], as an iteration's own reports it
int flush_update(gpslam_hip_handle *h) {
  if (!h->defer.update) return 0;
  h->defer.update = false;
  return launch_retract(h, LaunchMode{}, 2);
}

// One call of launch_factors as its parts below see it.  Every part takes the first free partial-sum slot and returns the next one, or
// a negative error code.  k_final_reduce adds the slots in index order, so the order of the parts -- GP priors, pose priors, velocity
// priors, between factors, the measurement kinds in FKind order, closures, state Gaussians, border Gaussians, landmark priors -- is
// the order of the sum.
struct FactorPass {
  gpslam_hip_handle *h;
  const LaunchMode &m;
  const LaunchForm form;
  const int pass;           // 0: Jacobian rows + error, 1: error only
  const bool e32;           // the error pass also stores its whitened errors as the fp32 right-hand side of the row tables
  // SE(3) chains whose GP priors travel as structured records: the interpolated measurement factors read their interval's record
  // (Jinv, Jinv Ad, the finite-difference block: MeasArgs::gps) instead of forming the same blocks again, so they run BEHIND k_lin
  bool meas_rec = false;
  hipStream_t side = nullptr;   // where the light kernels go: the handle's second stream if this launch forks, else its stream
  RowT *part(int off) const { return h->partial.as<RowT>() + off; }
};
// The merged launch applied a pending update: what k_meas beside it (d = 3 chains) needs to see the same states -- the update
// without a buffer to write (k_meas owns no state) and the buffers that launch READ (by now the handle's other pair)
struct PendBeside {
  bool applied = false;
  PendUpd u;
  const double *pose = nullptr, *vel = nullptr;
};

// GP priors, pose priors, velocity priors and between factors of a Jacobian pass over one Qc: ONE launch (k_lin).  Its extra
// workgroup reduces the previous retraction's maxima if they were deferred.  In its record forms on an fp64 handle it applies a
// pending update: every state goes into the other buffer, the two change places, and `beside` says so.
int launch_lin_merged(const FactorPass &c, int off, PendBeside &beside) {
  gpslam_hip_handle *h = c.h;
  LinArgs<RowT> la;
  const Deferred::Sums red = h->defer.dmax.take();
  la.red_in = red.n > 0 ? h->partial2.as<double>() : nullptr;
  la.red_n = red.n; la.red_out = h->scal.as<double>() + red.slot;
  la.gp = gp_args(h, c.m, c.part(off), c.e32, gp_ngroups(h) == 1 ? 0 : -1);
  la.nb_gp = nblocks(la.gp.count, 128);
  off += la.nb_gp;
  for (int kind = 0; kind < 3; kind++) {
    la.fac[kind] = fac_args(h, c.form, kind, c.part(off), c.e32);
    la.nb[kind] = nblocks(simple_set(h, kind).count(), 128);
    off += la.nb[kind];
  }
  const dim3 grid(la.nb_gp + la.nb[0] + la.nb[1] + la.nb[2] + (la.red_in ? 1 : 0)), t(128);
  const bool pend = kIsF64 && h->defer.update && la.gp.gps != nullptr;     // the previous iteration's update is applied by THIS launch
  if (pend) {
    const size_t np = (size_t)h->pd * h->stride * sizeof(double), nv = (size_t)h->d * h->stride * sizeof(double);
    HIPCHK(h->pose_bak.reserve(np));
    HIPCHK(h->vel_bak.reserve(nv));
    PendUpd u;
    u.dx = h->lv[0].x.as<double>(); u.pose_w = h->pose_bak.as<double>(); u.vel_w = h->vel_bak.as<double>();
    u.flag = h->flag.as<int>(); u.chart = h->cfg.chart; u.last = h->N - 1;
    la.gp.pend = u;
    for (int kind = 0; kind < 3; kind++) la.fac[kind].pend = u;
    beside.applied = true;
    beside.u = u;
    beside.u.pose_w = nullptr; beside.u.vel_w = nullptr;
    beside.pose = h->pose.as<double>(); beside.vel = h->vel.as<double>();
  }
  dispatch_mf(h->mf, [&](auto tag) {
    constexpr int MF = decltype(tag)::value;
    const bool vp = la.nb[1] > 0;
    if constexpr ((MF == POSE3 || MF == POSE2 || MF == ROT3 || MF == LINEAR3) && kIsF64) {
      if (la.gp.gps != nullptr) {      // structured GP records (never on a world-velocity chain: make_plan)
        if (vp) { h->census[GPSLAM_CENSUS_LIN_REC_VP]++; k_lin<RowT, MF, false, true, true><<<grid, t, 0, h->stream>>>(la); }
        else { h->census[GPSLAM_CENSUS_LIN_REC]++; k_lin<RowT, MF, false, false, true><<<grid, t, 0, h->stream>>>(la); }
        if (pend) {                    // the launch wrote every state into the other buffer: that one is current from here on
          h->census[GPSLAM_CENSUS_LIN_PEND]++;
          std::swap(h->pose, h->pose_bak);
          std::swap(h->vel, h->vel_bak);
          h->defer.update = false;
        }
        return;
      }
    }
    if (MF == POSE3 && h->vw) {
      if (vp) { h->census[GPSLAM_CENSUS_LIN_VW_VP]++; k_lin<RowT, MF, true, true><<<grid, t, 0, h->stream>>>(la); }
      else { h->census[GPSLAM_CENSUS_LIN_VW]++; k_lin<RowT, MF, true, false><<<grid, t, 0, h->stream>>>(la); }
    } else {
      if (vp) { h->census[GPSLAM_CENSUS_LIN_ROWS_VP]++; k_lin<RowT, MF, false, true><<<grid, t, 0, h->stream>>>(la); }
      else { h->census[GPSLAM_CENSUS_LIN_ROWS]++; k_lin<RowT, MF, false, false><<<grid, t, 0, h->stream>>>(la); }
    }
  });
  return off;
}

// The same factors where k_lin does not serve (an error pass, several Qc, no GP prior at all): one k_gp per Qc group, each with its
// U, then one k_simple per set that has factors, those on the side stream.  Deferred maxima of the previous retraction get a launch
// of their own in front.
int launch_lin_groups(const FactorPass &c, int off) {
  gpslam_hip_handle *h = c.h;
  const Deferred::Sums red = h->defer.dmax.take();
  if (red.n > 0) k_final_reduce<double><<<dim3(1), dim3(256), 0, h->stream>>>(h->partial2.as<double>(), red.n, h->scal.as<double>() + red.slot, 1);
  for (int grp = 0; grp < std::max(gp_ngroups(h), h->gp_left.empty() ? 0 : 1); grp++) {
    GpArgs<RowT> a = gp_args(h, c.m, c.part(off), c.e32, gp_ngroups(h) >= 1 ? grp : -1);
    const int nb = nblocks(a.count, 128);
    dispatch_mf(h->mf, [&](auto tag) {
      constexpr int MF = decltype(tag)::value;
      if (c.pass == 0) {
        h->census[GPSLAM_CENSUS_LIN_GROUPS]++;
        launch_gp_rows<MF>(h, a, nb);
      } else {
        k_gp<RowT, MF, 1><<<dim3(nb), dim3(128), 0, h->stream>>>(a);
      }
    });
    off += nb;
  }
  for (int kind = 0; kind < 3; kind++) {
    if (simple_set(h, kind).count() == 0) continue;
    FacArgs<RowT> a = fac_args(h, c.form, kind, c.part(off), c.e32);
    const int nb = nblocks(a.count, 128);
    dispatch_mf(h->mf, [&](auto tag) {
      constexpr int MF = decltype(tag)::value;
      const dim3 g(nb), t(128);
      if (c.pass == 0) {
        if (kind == 0) k_simple<RowT, MF, 0, true><<<g, t, 0, c.side>>>(a);
        else if (kind == 1) k_simple<RowT, MF, 1, true><<<g, t, 0, c.side>>>(a);
        else k_simple<RowT, MF, 2, true><<<g, t, 0, c.side>>>(a);
      } else {
        if (kind == 0) k_simple<RowT, MF, 0, false><<<g, t, 0, c.side>>>(a);
        else if (kind == 1) k_simple<RowT, MF, 1, false><<<g, t, 0, c.side>>>(a);
        else k_simple<RowT, MF, 2, false><<<g, t, 0, c.side>>>(a);
      }
    });
    off += nb;
  }
  return off;
}

// GPInterpolatedGPSFactorPose3 as 16-double lines: fp64 only (Plan::lines; make_plan never selects them on an fp32 handle, whose
// half therefore holds no form of k_gps_lines)
template <typename R> void launch_gps_lines_k(int32_t *cen, const MeasArgs<R> &a, int nb, hipStream_t st) {
  if constexpr (std::is_same<R, double>::value) {
    cen[GPSLAM_CENSUS_GPS_LINES]++;
    if (a.aidx != nullptr) k_gps_lines<kGpsLinesWaves, true><<<dim3(nb), dim3(128), 0, st>>>(a);   // (round 6: a kernel written for its register count)
    else k_gps_lines<kGpsLinesWaves, false><<<dim3(nb), dim3(128), 0, st>>>(a);
  }
}

// The measurement kinds in FKind order, one k_meas each on the side stream -- interpolated GPS as 16-double lines (k_gps_lines) where
// the launch's form says so
int launch_meas_kinds(const FactorPass &c, int off, const PendBeside &beside) {
  gpslam_hip_handle *h = c.h;
  for (int fk = 0; fk < kNumMeasKinds; fk++) {
    MeasSet &s = h->ms[fk];
    if (s.count() == 0) continue;
    MeasArgs<RowT> a = meas_args(h, fk);
    a.rob = s.rob.empty() ? nullptr : s.d_rob.as<double>();
    a.out_w = (c.m.weights && a.rob) ? s.d_w.as<RowT>() : nullptr;
    a.rowLR = h->rowLR.as<RowT>(); a.rowE = h->rowE.as<RowT>(); a.rowM = h->rowM.as<RowT>(); a.rowLm = h->rowLm.as<int>();
    a.partial = c.part(off); a.rowE32 = c.e32 ? h->rowE.as<float>() : nullptr;
    if (c.meas_rec) { a.gps = h->gps.as<RowT>(); a.gpidx = h->gpidx.as<int>(); }
    if (beside.applied && !c.meas_rec) {   // beside k_lin, not behind it: the old buffer + the update
      if (!s.two) return fail(h, GPSLAM_E_INVALID, "internal: a pending update met a measurement kind that cannot apply it");
      a.pose = beside.pose; a.vel = beside.vel; a.pend = beside.u;
    }
    const int nb = nblocks(a.count, 128);
    off += nb;
    if constexpr (kIsF64) {
      if (c.meas_rec && c.form.lines && fk == FK_INTERP_GPS) {   // 16-double lines for k_fused_level0<4> instead of 24-column rows
        a.rowI = h->rowI.as<RowT>(); a.row0 = s.d_irow0.as<int>();
        a.rowLR = nullptr; a.rowE = nullptr; a.rowM = nullptr; a.rowLm = nullptr;
        launch_gps_lines_k(h->census.v, a, nb, c.side);
        continue;
      }
    }
    dispatch_mf(h->mf, [&](auto tag) {
      constexpr int MF = decltype(tag)::value;
      dispatch_fk(fk, [&](auto ftag) {
        constexpr int FK = decltype(ftag)::value;
        if (c.pass == 0) {
          if (FK == FK_INTERP_GPS) h->census[a.gps != nullptr ? GPSLAM_CENSUS_MEAS_REC : GPSLAM_CENSUS_MEAS_SELF]++;
          k_meas<RowT, MF, FK, true><<<dim3(nb), dim3(128), 0, c.side>>>(a);
        }
        else k_meas<RowT, MF, FK, false><<<dim3(nb), dim3(128), 0, c.side>>>(a);
      });
    });
  }
  return off;
}

// What has no row of the chain's tables to itself, on the side stream (fp64 handles only; RowT == Real == double where they run):
// loop closures -- records [A_i | A_j | r] in a Jacobian pass, and their error (one slot); joint Gaussians on one state
// (fixedlag.hip: rows [A | 0] and their error); joint Gaussians on one state and the landmarks (residuals and their error, one
// slot); landmark priors (no Jacobian rows: on an fp32 handle their error belongs to the fp64 error pass alone)
int launch_other_factors(const FactorPass &c, int off) {
  gpslam_hip_handle *h = c.h;
  if (kIsF64 && h->clo.n > 0) {
    closures_eval(h, c.m, c.pass, reinterpret_cast<double *>(c.part(off)), c.side);
    off += 1;
  }
  if (kIsF64 && h->sg.count() > 0) {
    state_gauss_eval(h, c.pass, reinterpret_cast<double *>(c.part(off)), c.side);
    off += nblocks(h->sg.count(), 128);
  }
  if (kIsF64 && h->bg.count() > 0) {
    border_gauss_eval(h, c.pass, reinterpret_cast<double *>(c.part(off)), c.side);
    off += 1;
  }
  if (kIsF64 && h->lpri.count() > 0 && h->fs.active) {   // tens of thousands of landmark priors: grid-stride, one partial per block
    const int nbl = std::min(nblocks(h->lpri.count(), 256), 256);
    fs_lmprior_err(h, nbl, c.part(off), c.side);
    off += nbl;
  } else if (kIsF64 && h->lpri.count() > 0) {
    LmArgs<Real, RowT> a = lm_args(h, 0.0);
    a.partial = reinterpret_cast<Real *>(c.part(off));
    k_lmprior_err<Real, RowT><<<dim3(1), dim3(128), 0, c.side>>>(a);
    off += 1;
  }
  return off;
}

// pass 0: Jacobian rows + error, 1: error only.  Error partial sums land in h->partial, reduced into scal[slot] (or left to this
// iteration's k_retract: LaunchMode::defer_error).  An fp32 handle's residual is always evaluated in fp64: its pass 1 IS impl64's, and
// its pass 0 ends in impl64's pass 1 with e32 -- whitened errors into the fp32 rowE, the error into scal[slot].
int launch_factors(gpslam_hip_handle *h, const LaunchMode &m, int pass, int slot, bool e32) {
  if (!kIsF64 && pass == 1) return impl64::launch_factors(h, m, 1, slot, false);
  FactorPass c{h, m, launch_form(h, m), pass, e32};
  bool any_meas = h->lpri.count() > 0;
  for (const MeasSet &s : h->ms) any_meas = any_meas || s.count() > 0;
  const bool chain = !h->gp_left.empty();
  const bool merged = pass == 0 && chain && gp_ngroups(h) <= 1;   // k_lin; else one launch per Qc group and per set
  c.meas_rec = pass == 0 && c.form.gp == GpForm::Se3Rec && any_meas;
  int rc;
  if (h->defer.update && !(merged && c.form.gp != GpForm::Rows)) {   // (defensive: an update is pending and this launch cannot apply it)
    h->census[GPSLAM_CENSUS_FLUSH]++;
    if ((rc = flush_update(h))) return rc;
  }
  // fork: the factor kernels are independent of one another (disjoint rows, disjoint partial sums) -- unless k_meas reads k_lin's records
  const bool fork = pass == 0 && chain && h->aux_stream != nullptr && (any_meas || !merged) && !c.meas_rec && h->N >= kForkMinStates && h->fs.active;
  c.side = fork ? h->aux_stream : h->stream;
  if (fork) {
    HIPCHK(hipEventRecord(h->ev_fork, h->stream));
    HIPCHK(hipStreamWaitEvent(h->aux_stream, h->ev_fork, 0));
  }
  PendBeside beside;
  int off = merged ? launch_lin_merged(c, 0, beside) : launch_lin_groups(c, 0);
  if (off >= 0) off = launch_meas_kinds(c, off, beside);
  if (off >= 0) off = launch_other_factors(c, off);
  if (off < 0) return off;
  if (fork) {   // joined before the reduction
    HIPCHK(hipEventRecord(h->ev_join, h->aux_stream));
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));
  }
  if (kIsF64 && m.defer_error) h->defer.err = {off, slot};     // summed by the extra workgroup of this iteration's k_retract
  else if (kIsF64) k_final_reduce<RowT><<<dim3(1), dim3(256), 0, h->stream>>>(c.part(0), off, h->scal.as<double>() + slot, 0);
  HIPCHK(hipGetLastError());
  return kIsF64 ? 0 : impl64::launch_factors(h, m, 1, slot, true);   // fp32 rows are in place; now the fp64 residual
}

// pass (closures in column passes, clo.P > 1): which slice of the closures' columns the records take; pass == clo.P: the final
// pass, whose right-hand sides are U^T Y alone
int launch_assemble(gpslam_hip_handle *h, const LaunchMode &m, bool save_g, int pass) {
  AsmArgs<Real, RowT> a;
  a.N = h->N; a.R = h->R;
  a.rowptr = h->rowptr.as<int>();
  a.rowLR = h->rowLR.as<RowT>(); a.rowE = h->rowE.as<RowT>();
  a.crowptr = h->crowptr.as<int>(); a.rowC = h->rowC.as<RowT>(); a.rowCE = h->rowCE.as<RowT>();
  const bool border = h->nl > 0 && !h->fs.active;   // landmark columns ride in the records only with the dense border
  a.rowM = border ? h->rowM.as<RowT>() : nullptr;
  a.rowLm = border ? h->rowLm.as<int>() : nullptr;
  a.ld = h->ld;
  a.blk = h->lv[0].blk.as<Real>();
  a.gsave = save_g ? h->gsave.as<Real>() : nullptr;
  a.halo_add = has_right_rank(h) ? h->halo_add.as<Real>() : nullptr;
  const bool rec3 = gp_form(h, m) == GpForm::D3Rec;
  int rc;
  if (rec3 && (rc = refresh_dU(h))) return rc;
  a.gps3 = rec3 ? h->gps.as<Real>() : nullptr;
  a.gpidx = h->gpidx.as<int>(); a.gp_count = (int)h->gp_left.size(); a.Ud = h->dU.as<Real>();
  const int nstates = h->N + (a.halo_add ? 1 : 0);
  dispatch_b(h->b, [&](auto tag) {
    constexpr int BB = decltype(tag)::value;
    const int waves = nblocks(nstates, 64 / BB - 1);
    k_assemble_ghost<Real, BB, 4, RowT><<<dim3(nblocks(waves, 4)), dim3(256), 0, h->stream>>>(a);   // 1 / 8 / 16 waves per block measured slower
  });
  if (h->clo.n > 0) closures_inject(h, save_g, pass);   // the closures' columns of U^T into the records of their states
  if (kIsF64 && h->bg.count() > 0) border_gauss_inject(h, save_g);   // the border Gaussians' blocks into the records of their states
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_fwd(gpslam_hip_handle *h, const LaunchMode &m, const FwdArgs<Real> &a, int grid) {
  const bool fast = (4 * h->b + 2 * h->R <= 64);   // room for the separator sums in spare lanes
  // level 0 of a Pose3 chain without landmark columns: four chunks per wave, panel rows in lanes
  if (m.fused && !a.no_sep && !a.add) {
    FusedArgs<Real, RowT> u;
    u.f = a;
    u.rowptr = h->rowptr.as<int>(); u.rowLR = h->rowLR.as<RowT>(); u.rowE = h->rowE.as<RowT>();
    u.crowptr = h->crowptr.as<int>(); u.rowC = h->rowC.as<RowT>(); u.rowCE = h->rowCE.as<RowT>();
    int rc;
    if (gp_form(h, m) != GpForm::Rows && (rc = refresh_dU(h))) return rc;   // (set_qc after compile(): the diagonal form may come or go)
    const LaunchForm form = launch_form(h, m);
    u.gps = form.gp != GpForm::Rows ? h->gps.as<Real>() : nullptr;
    u.gp_count = (int)h->gp_left.size();
    u.gpidx = h->gpidx.as<int>();
    u.brec = form.btw_rec ? h->brec.as<Real>() : nullptr;
    u.btwidx = h->btwidx.as<int>(); u.btw_count = h->btw.count();
    u.odd_rows = h->plan.odd_rows;
    if constexpr (kIsF64) {
      if (form.lines) { u.rowI = h->rowI.as<Real>(); u.irowptr = h->irowptr.as<int>(); }   // k_fused_level0<4>
    }
    u.gsave = m.gsave ? h->gsave.as<Real>() : nullptr;
    u.gsave2 = m.gsave ? h->gsave2.as<Real>() : nullptr;
    u.simd_cnt = h->simd_cnt.as<int>();
    u.Ud = h->dU.as<Real>();
    u.u_diag = form.dg ? 1 : 0;   // a diagonal chol_upper(Qc^-1) (isotropic / diagonal Qc) takes the assembly wave's shorter form
#ifdef GPS_TRACE_FUSED
    h->dbg_trace_waves = nblocks(grid, 4) * 2;
    (void)h->dbg_trace.reserve((size_t)h->dbg_trace_waves * 64 * 8);
    (void)hipMemsetAsync(h->dbg_trace.p, 0, (size_t)h->dbg_trace_waves * 64 * 8, h->stream);
    u.trace = h->dbg_trace.as<unsigned long long>();
#endif
    launch_fused_k(h->census.v, h->b, form.sv, form.dg, u, nblocks(grid, 4), h->stream, m.l0_events ? h->ev_l0a : nullptr, m.l0_events ? h->ev_l0b : nullptr);
    return 0;
  }
  if (h->plan.rows() && !a.no_sep && !a.add) {
    launch_rows_k(h->census.v, h->b, a, nblocks(grid, 4), h->stream);
    return 0;
  }
  dispatch_b(h->b, [&](auto tag) {
    constexpr int BB = decltype(tag)::value;
    // (census: a level with addends is a level above 0; without them, the top solve where no separator is kept, else level 0)
    h->census[a.add ? GPSLAM_CENSUS_UPPER_CHUNK : (a.no_sep ? GPSLAM_CENSUS_TOP_CHUNK : GPSLAM_CENSUS_L0_COLUMN)]++;
    if (fast && !a.add && !a.no_sep) h->census[GPSLAM_CENSUS_L0_COLUMN_FAST]++;
    if (fast) k_chunk_forward<Real, BB, true><<<dim3(grid), dim3(64), 0, h->stream>>>(a);
    else k_chunk_forward<Real, BB, false><<<dim3(grid), dim3(64), 0, h->stream>>>(a);
  });
  return 0;
}
void launch_bwd(gpslam_hip_handle *h, const BwdArgs<Real> &a, int grid) {
  // chains without landmark columns: the row-layout kernel, four chunks per wave (the column-layout plan keeps the generic one)
  if (a.R == 1 && h->plan.rows()) { launch_bwd_rows_k(h->census.v, h->b, a, nblocks(grid, 4), h->stream); return; }
  dispatch_b(h->b, [&](auto tag) {
    constexpr int BB = decltype(tag)::value;
    h->census[GPSLAM_CENSUS_BWD_CHUNK]++;
    // 16-byte pieces per lane per record: 3 wave loads cover 2 b^2 + b R <= 384 doubles, 5 cover every admissible R
    if (2 * BB * BB + BB * h->R <= 384) k_chunk_backward<Real, BB, 3><<<dim3(grid), dim3(64), 0, h->stream>>>(a);
    else k_chunk_backward<Real, BB, 5><<<dim3(grid), dim3(64), 0, h->stream>>>(a);
  });
}

// Level 1 as groups of four (Plan::tail_fold): a fused level 0 reduces its four chunk separators in its own tail; the unfused
// level-0 kernels leave that level to a launch of upper.hip's kernel with G = 4.
bool tail_now(const gpslam_hip_handle *h, const LaunchMode &m) { return h->plan.tail_fold && m.fused; }

// The forward elimination of level l as one of the chunk kernels of this file runs it, and its grid.  Unsharded: the last level is
// the top solve.  Sharded: every level keeps its first block as separator; the last level reduces to the interface record.
FwdArgs<Real> fwd_args(gpslam_hip_handle *h, const LaunchMode &m, int l, double lambda, int &grid) {
  const size_t BS = (size_t)2 * h->b * h->b + (size_t)h->b * h->R, AS = (size_t)h->b * h->b + (size_t)h->b * h->R;
  Level &v = h->lv[l];
  const bool last = (l == (int)h->lv.size() - 1);
  FwdArgs<Real> a;
  a.blk = v.blk.as<Real>();
  a.add = (l > 0) ? v.add.as<Real>() : nullptr;
  a.n = v.n; a.R = h->R;
  a.m = last ? v.n : v.m;
  a.lambda = (l == 0) ? (Real)lambda : Real(0);
  a.flag = h->flag.as<int>();
  a.remote_add = nullptr;
  a.l1_blk = nullptr; a.tail = 0;
  grid = last ? 1 : v.nch;
  if (!sharded(h)) {
    a.up_blk = last ? nullptr : h->lv[l + 1].blk.as<Real>();
    a.up_add = last ? nullptr : h->lv[l + 1].add.as<Real>();
    a.no_sep = last ? 1 : 0;
    a.last_has_right = 0;
    if (l == 0 && tail_now(h, m)) {   // the fused kernel reduces its four separators itself: its output is level 2's input
      a.tail = 1;
      a.l1_blk = h->lv[1].blk.as<Real>();
      a.up_blk = h->lv[2].blk.as<Real>();
      a.up_add = h->lv[2].add.as<Real>();
    }
  } else {
    a.up_blk = last ? h->iface_send.as<Real>() : h->lv[l + 1].blk.as<Real>();
    // the interface record is [blk (BS) | addend slot 1 (AS)]; addend slot 0 is unused, so point one slot back
    a.up_add = last ? h->iface_send.as<Real>() + BS - AS : h->lv[l + 1].add.as<Real>();
    a.no_sep = 0;
    a.last_has_right = has_right_rank(h) ? 1 : 0;
    if (a.last_has_right) a.remote_add = (l == 0) ? h->halo_add.as<Real>() : v.add.as<Real>() + (size_t)v.n * AS;
  }
  return a;
}
// Forward elimination through the local levels.
int launch_forward(gpslam_hip_handle *h, const LaunchMode &m, double lambda) {
  const int nl = (int)h->lv.size();
  const bool sh = sharded(h);
  const size_t BS = (size_t)2 * h->b * h->b + (size_t)h->b * h->R, AS = (size_t)h->b * h->b + (size_t)h->b * h->R;
  int rc;
  for (int l = 0; l < nl; l++) {
    Level &v = h->lv[l];
    const bool last = (l == nl - 1);
    if (h->plan.upper_cr && l >= 1) {   // (the last level also solves and back-substitutes itself)
      if (l == 1 && tail_now(h, m)) continue;   // done in the tail of the level-0 kernel
      UpFwdArgs u;
      u.blk = v.blk.as<double>(); u.add = v.add.as<double>();
      u.up_blk = last ? nullptr : h->lv[l + 1].blk.as<double>();
      u.up_add = last ? nullptr : h->lv[l + 1].add.as<double>();
      u.x = v.x.as<double>(); u.n = v.n; u.ext = 0; u.flag = h->flag.as<int>();
      if (sh) {   // every level keeps its first block; the last one (a single group) leaves the interface record
        u.ext = has_right_rank(h) ? 1 : 0;     // [blk (BS) | addend slot 1 (AS)]: slot 0 is unused, so point one slot back
        if (last) { u.up_blk = h->iface_send.as<double>(); u.up_add = h->iface_send.as<double>() + BS - AS; }
      }
      h->census[GPSLAM_CENSUS_UPPER_CR]++;
      const int e = upper_forward(h->b, v.m, last && !sh, u, h->stream);
      if (e) { h->err = std::string("upper_forward: ") + hipGetErrorString((hipError_t)e); return GPSLAM_E_HIP; }
      continue;
    }
    int grid;
    const FwdArgs<Real> a = fwd_args(h, m, l, lambda, grid);
    if ((rc = launch_fwd(h, m, a, grid))) return rc;
    if (l == 0 && m.stamp_l0) HIPCHK(hipEventRecord(h->ev[5], h->stream));
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// Back-substitution through the local levels; xtop = separator solutions for the last level (sharded) or null
// Level 1 as groups of four whose groups are exactly the waves of the row-layout level-0 back-substitution (four chunks per wave):
// that kernel then solves its group itself and the launch of k_multi_backward<B, 4> is dropped (Plan::fold_tail_bwd: unsharded fp64
// chains; A/B on one box: 0.3066 vs 0.3118 ms per iteration at 1e5 Pose3 states, 2.43-2.45 vs 2.45-2.46 ms at 1e6).
// Layout contract (ADVICE r4): whichever kernel reduces the level of groups of four -- the tail of k_fused_level0 (default) or
// upper.hip's k_multi_forward<B, 4> (GPSLAM_PLAN_UNFUSED_LEVEL0, the Levenberg-Marquardt trials of the unfused pair) -- leaves that
// level's factor records in lv[1].blk as column-major [V | U | Y] (the one record layout of the solver: BwdArgs::blk, UpBwdArgs::blk)
// and the solutions of the groups' first blocks in lv[2].x; k_chunk_backward_rows reads exactly those two through BwdArgs::l1_blk /
// l1_xup.  tests/test_gpu_switches.py runs both producers against the oracle (chains whose lv[1].n % 4 is 1, 2 and 3 included).
BwdArgs<Real> bwd_args(gpslam_hip_handle *h, int l, const Real *xtop, int &grid) {
  Level &v = h->lv[l];
  const bool last = (l == (int)h->lv.size() - 1);
  BwdArgs<Real> a;
  a.blk = v.blk.as<Real>(); a.x = v.x.as<Real>();
  a.n = v.n; a.R = h->R;
  a.m = last ? v.n : v.m;
  grid = last ? 1 : v.nch;
  if (!sharded(h)) {
    a.xup = last ? nullptr : h->lv[l + 1].x.as<Real>();
    a.no_sep = last ? 1 : 0; a.last_has_right = 0;
    if (l == 0 && h->plan.fold_tail_bwd) {
      a.l1_blk = h->lv[1].blk.as<Real>(); a.l1_xup = h->lv[2].x.as<Real>(); a.l1_n = h->lv[1].n;
    }
  } else {
    a.xup = last ? xtop : h->lv[l + 1].x.as<Real>();
    a.no_sep = 0; a.last_has_right = has_right_rank(h) ? 1 : 0;
  }
  return a;
}
int launch_backward(gpslam_hip_handle *h, const Real *xtop) {
  const int nl = (int)h->lv.size();
  const bool sh = sharded(h);
  for (int l = nl - 1; l >= 0; l--) {
    Level &v = h->lv[l];
    const bool last = (l == nl - 1);
    if (h->plan.upper_cr && l >= 1) {
      if (last && !sh) continue;   // solved inside its forward launch
      if (l == 1 && h->plan.fold_tail_bwd) continue;   // the level of groups of four: k_chunk_backward_rows solves its own group
      UpBwdArgs u;
      u.blk = v.blk.as<double>(); u.x = v.x.as<double>(); u.n = v.n;
      u.xup = last ? xtop : h->lv[l + 1].x.as<double>();
      u.ext = (sh && has_right_rank(h)) ? 1 : 0;
      h->census[GPSLAM_CENSUS_UPPER_BWD]++;
      const int e = upper_backward(h->b, v.m, u, h->stream);
      if (e) { h->err = std::string("upper_backward: ") + hipGetErrorString((hipError_t)e); return GPSLAM_E_HIP; }
      continue;
    }
    int grid;
    const BwdArgs<Real> a = bwd_args(h, l, xtop, grid);
    launch_bwd(h, a, grid);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// landmark Schur complement, landmark solve, pose correction (nl > 0)
// Landmark border in two halves: (a) this handle's contribution to the Schur complement [S | gL] -- summed over the
// ranks by the caller when the chain is sharded -- and (b) the landmark solve and the correction of the chain update.
int launch_landmarks_reduce(gpslam_hip_handle *h, double lambda) {
  if (h->nl <= 0) return 0;
  LmArgs<Real, RowT> a = lm_args(h, lambda);
  if (h->nlmrows > 0) k_lm_t<Real, RowT><<<dim3(nblocks(h->nlmrows * h->R, 128)), dim3(128), 0, h->stream>>>(a);
  if (h->nlmchunks > 0) k_lm_reduce_part<Real, RowT><<<dim3(h->nlmchunks), dim3(256), 0, h->stream>>>(a);
  k_lm_reduce<Real, RowT><<<dim3(h->nl * h->R), dim3(64), 0, h->stream>>>(a);
  if (kIsF64 && h->bg.count() > 0) border_gauss_schur(h);   // the border Gaussians have no rows: their share of [S | gL]
  HIPCHK(hipGetLastError());
  return 0;
}
int launch_landmarks_solve(gpslam_hip_handle *h, double lambda) {
  if (h->nl <= 0) return 0;
  LmArgs<Real, RowT> a = lm_args(h, lambda);
  k_lm_solve<Real, RowT><<<dim3(1), dim3(64), 0, h->stream>>>(a);
  k_lm_correct<Real, RowT><<<dim3(nblocks(h->N * h->b, 256)), dim3(256), 0, h->stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}
int launch_landmarks(gpslam_hip_handle *h, double lambda) {
  int rc = launch_landmarks_reduce(h, lambda);
  return rc ? rc : launch_landmarks_solve(h, lambda);
}

// A piece of a split chain (the segmented landmark elimination is fatsep.hip's): linearisation, assembly, the forward half down to
// the piece's two end blocks, and the interface record.
// lm_trial: the rows are those of the linearisation point (gpslam_hip_lm_begin); the assembly also stores the gradient.
// clear_flag = false: inside a multi-iteration run (dist_run_gn) the non-positive-pivot flag is sticky
int fs_split_phase1(gpslam_hip_handle *h, double lambda, bool lm_trial, bool clear_flag) {
  int rc;
  h->ph_lambda = lambda;
  if (clear_flag) HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  if (!lm_trial && (rc = launch_factors(h, LaunchMode{}, 0, 0))) return rc;
  if ((rc = launch_assemble(h, LaunchMode{}, lm_trial))) return rc;
  if ((rc = fs_forward(h, lambda))) return rc;
  return fs_pack_record(h);
}

// Closures in column passes (clo.P > 1): the caller's assembly carried slice 0.  Every pass is the same factorisation at the same
// lambda; the records are reassembled in front of each one because the elimination works in place.  The marginals run the same
// passes at lambda = 0 with m.keep_z (every pass's slice of Z = A^-1 U^T copied into h->mg.Z behind its backward sweep) and
// m.lm_reduce_only.  Leaves W = U [X | Z] in clo.W and the corrected landmark columns in the leading columns of the level-0 solution.
int launch_solve_passes(gpslam_hip_handle *h, const LaunchMode &m, double lambda) {
  int rc;
  const int P = h->clo.P;
  LaunchMode later = m;       // (a timed iteration stamps the level-0 launch of pass 0 alone)
  later.stamp_l0 = false;
  for (int p = 0; p < P; p++) {
    if (p > 0 && (rc = launch_assemble(h, m, false, p))) return rc;
    if ((rc = launch_forward(h, p == 0 ? m : later, lambda))) return rc;
    if ((rc = launch_backward(h, nullptr))) return rc;
    closures_collect(h, p, m.keep_z);   // (behind the last pass: the wide solve for Y)
  }
  if ((rc = launch_assemble(h, m, false, P))) return rc;
  if ((rc = launch_forward(h, later, lambda))) return rc;
  if ((rc = launch_backward(h, nullptr))) return rc;
  if ((rc = closures_add(h))) return rc;
  return m.lm_reduce_only ? launch_landmarks_reduce(h, lambda) : launch_landmarks(h, lambda);
}

// The solve behind an assembly: forward, backward, the closures' correction, the landmarks.  With m.lm_reduce_only (the marginals, the
// evidence: at lambda = 0) it leaves the solver's right-hand sides -- the closure columns Z = A^-1 J_c^T, the landmark columns
// corrected for the closures, the landmark Schur complement S of the whole chain -- and the states stay.
int launch_solve(gpslam_hip_handle *h, const LaunchMode &m, double lambda) {
  int rc;
  if (h->fs.active) return fs_solve(h, lambda);
  if (h->clo.P > 1) return launch_solve_passes(h, m, lambda);
  if ((rc = launch_forward(h, m, lambda))) return rc;
  if ((rc = launch_backward(h, nullptr))) return rc;
  if ((rc = closures_correct(h))) return rc;
  return m.lm_reduce_only ? launch_landmarks_reduce(h, lambda) : launch_landmarks(h, lambda);
}

// k_retract over the local states: its arguments and its grid (one workgroup more when this iteration's error partial sums are
// still waiting in `partial`: the launch takes them along)
RetractArgs<Real> retract_args(gpslam_hip_handle *h, int &grid) {
  RetractArgs<Real> a;
  a.pose = h->pose.as<double>(); a.vel = h->vel.as<double>(); a.stride = h->stride; a.N = h->N; a.R = h->R;
  a.chart = h->cfg.chart; a.first = 0; a.x = h->lv[0].x.as<Real>(); a.partial = h->partial2.as<Real>(); a.flag = h->flag.as<int>();
  const Deferred::Sums red = h->defer.err.take();
  a.red_in = red.n > 0 ? h->partial.as<double>() : nullptr; a.red_n = red.n; a.red_out = h->scal.as<double>() + red.slot;
  grid = nblocks(h->N, 128) + (red.n > 0 ? 1 : 0);
  return a;
}
void launch_retract_k(gpslam_hip_handle *h) {
  int grid;
  const RetractArgs<Real> a = retract_args(h, grid);
  h->census[GPSLAM_CENSUS_RETRACT]++;
  dispatch_mf(h->mf, [&](auto tag) {
    constexpr int MF = decltype(tag)::value;
    k_retract<Real, MF><<<dim3(grid), dim3(128), 0, h->stream>>>(a);
  });
}
// x <- x (+) delta for the local states (and landmarks); scal[slot] = |delta|_inf
int launch_retract(gpslam_hip_handle *h, const LaunchMode &m, int slot) {
  const int nb = nblocks(h->N, 128);
  launch_retract_k(h);
  if (m.defer_maxima && h->nl == 0) h->defer.dmax = {nb, slot};   // reduced by the next linearisation's launch
  else k_final_reduce<Real><<<dim3(1), dim3(256), 0, h->stream>>>(h->partial2.as<Real>(), nb, h->scal.as<double>() + slot, 1);
  if (h->nl > 0 && h->fs.active) fs_lm_update(h, slot, h->stream);
  else if (h->nl > 0) {
    LmArgs<Real, RowT> la = lm_args(h, 0.0);
    k_lm_update<Real, RowT><<<dim3(1), dim3(64), 0, h->stream>>>(la, h->scal.as<double>() + slot);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// The mode of one Gauss-Newton iteration (enqueue_gn; collect_timing reads its level-0 stamps).  Deferred reductions: chains
// without landmarks on an unsharded handle (the landmark update folds its maximum into the same slot; sharded iterations do not
// come through here); eval_after = false: the next iteration's k_lin follows and reduces the retraction's maxima.
LaunchMode gn_mode(const gpslam_hip_handle *h, bool timed, bool eval_after) {
  LaunchMode m = level0_mode(h);
  m.defer_error = h->nl == 0 && !h->fs.active && kIsF64;
  m.defer_maxima = m.defer_error && !eval_after;
  m.stamp_l0 = timed && !h->fs.active;
  m.l0_events = m.stamp_l0 && m.fused && h->l0_stamps && h->ev_l0a != nullptr;
  return m;
}
// one Gauss-Newton iteration enqueued on the stream (no host sync); records phase events when timed.
// eval_after = false skips the error-only pass over the retracted state: inside a fixed-count run the next
// iteration's linearisation evaluates exactly that error anyway (scal[0]), so it is computed once, not twice.
int enqueue_gn(gpslam_hip_handle *h, const LaunchMode &m, double lambda, bool timed, bool eval_after, bool defer_retract) {
  int rc;
  if (timed) HIPCHK(hipEventRecord(h->ev[0], h->stream));
  if ((rc = launch_factors(h, m, 0, 0))) { h->defer.err.n = 0; return rc; }
  if (timed) HIPCHK(hipEventRecord(h->ev[1], h->stream));
  if (!m.fused && (rc = launch_assemble(h, m, false))) return rc;   // (fused: the assembly happens inside the level-0 elimination)
  if (timed) HIPCHK(hipEventRecord(h->ev[2], h->stream));
  if ((rc = launch_solve(h, m, lambda))) return rc;
  if (timed) HIPCHK(hipEventRecord(h->ev[3], h->stream));
  if (defer_retract) {                                  // run_gn, not the last iteration: the NEXT k_lin applies this update
    h->defer.update = true;
    if (timed) HIPCHK(hipEventRecord(h->ev[4], h->stream));
    return 0;
  }
  if ((rc = launch_retract(h, m, 2))) return rc;
  if (eval_after && (rc = launch_factors(h, LaunchMode{}, 1, 1))) return rc;
  if (timed) HIPCHK(hipEventRecord(h->ev[4], h->stream));
  return 0;
}

// scal[slot] = sum_i x[i] * y[i]
int launch_dot(gpslam_hip_handle *h, const Real *x, const Real *y, int n, int slot) {
  const int nb = nblocks(n, 256);
  k_dot<Real><<<dim3(nb), dim3(256), 0, h->stream>>>(x, y, n, h->partial.as<Real>());
  k_final_reduce<Real><<<dim3(1), dim3(256), 0, h->stream>>>(h->partial.as<Real>(), nb, h->scal.as<double>() + slot, 0);
  HIPCHK(hipGetLastError());
  return 0;
}

// scal[s0] = x . y0, scal[s1] = x . y1 (y1 may be null: then s1 < 0), scal[s2] = x . x -- two launches instead of six,
// same partial sums in the same order as three launch_dot calls
int launch_dot3(gpslam_hip_handle *h, const Real *x, const Real *y0, const Real *y1, int n, int s0, int s1, int s2) {
  const int nb = nblocks(n, 256);
  k_dot3<Real><<<dim3(nb), dim3(256), 0, h->stream>>>(x, y0, y1, n, h->partial.as<Real>());
  k_final_reduce3<Real><<<dim3(3), dim3(256), 0, h->stream>>>(h->partial.as<Real>(), nb, h->scal.as<double>(), s0, y1 ? s1 : -1, s2);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- compile(): its steps, in the order gpslam_hip_compile calls them

// factors were range-checked against the N and L of the moment they were added; set_states / set_landmarks may
// have shrunk either since (ADVICE r1): re-validate every stored index before it is used to size or index anything
int check_stored_indices(gpslam_hip_handle *h) {
  const int N = h->N, ml = max_left(h);
  auto bad = [](const std::vector<int32_t> &v, int hi) { for (int32_t i : v) if (i < 0 || i > hi) return true; return false; };
  if (bad(h->gp_left, ml) || bad(h->btw.idx, ml) || bad(h->pri.idx, N - 1) || bad(h->vpri.idx, N - 1) || bad(h->lpri.idx, h->L - 1))
    return fail(h, GPSLAM_E_INVALID, "a stored factor refers to a state / landmark that no longer exists (set_states / set_landmarks shrank the problem)");
  for (const MeasSet &s : h->ms)
    if (bad(s.idx, s.two ? ml : N - 1) || (s.haslm && bad(s.lm, h->L - 1)))
      return fail(h, GPSLAM_E_INVALID, "a stored measurement factor refers to a state / landmark that no longer exists");
  if (bad(h->sg.idx, N - 1)) return fail(h, GPSLAM_E_INVALID, "a stored state Gaussian refers to a state that no longer exists (set_states shrank the problem)");
  if (bad(h->bg.idx, N - 1)) return fail(h, GPSLAM_E_INVALID, "a stored border Gaussian refers to a state that no longer exists (set_states shrank the problem)");
  if (h->bg.count() > 0 && h->bg.nl != h->L * h->ld)
    return fail(h, GPSLAM_E_INVALID, "a stored border Gaussian spans another number of landmarks than the handle has (set_landmarks changed it)");
  return 0;
}

// The right-hand sides of the chain solver, R = [update | landmark columns | closure columns], and where the landmarks go.
// Up to kMaxRhs - 1 landmark columns ride through the whole chain solver as extra right-hand sides (the dense border, Plaza's
// handful of beacons).  More than that -- config 4's 5e4 locally visible landmarks -- go through the segmented elimination with
// fat separators (fatsep.hpp); force_segmented = 1 forces that path for any landmark count.
int choose_landmark_path(gpslam_hip_handle *h, bool &segmented) {
  const int N = h->N, d = h->d, b = h->b;
  h->nl = h->L * h->ld;
  h->clo.n = h->clo.fac.count();
  h->clo.nc = h->clo.n * d;
  for (int k = 0; k < h->clo.n; k++)
    if (h->clo.fac.idx[k] >= N || h->clo.second[k] >= N)
      return fail(h, GPSLAM_E_INVALID, "a stored loop closure refers to a state that no longer exists (set_states shrank the problem)");
  h->clo.slice = h->clo.n;
  h->clo.P = h->clo.n > 0 ? 1 : 0;
  bool passes = false;
  // closures in column passes (gpslam_hip_set_closure_passes, max_passes >= 2; unsharded fp64 handles, the others are refused below):
  // slices of w closures, R = 1 + nl + w d.  A graph that fits one pass keeps today's path and today's R
  if (h->clo.n > 0 && h->clo.max_passes >= 2 && kIsF64 && !sharded(h) && h->cfg.force_segmented != 1 && !h->fs.split) {
    const int room = std::min(kMaxRhs, 64 - 3 * b) - 1 - h->nl;   // 1 + nl + w d <= 28 and 3 b + R <= 64
    const int fit = room > 0 ? room / d : 0;
    int w = h->clo.per_pass > 0 ? h->clo.per_pass : fit;
    if (fit < 1) return fail(h, GPSLAM_E_UNSUPPORTED, "loop closures in column passes: the landmark columns leave no room for a closure (1 + landmarks * landmark_dim + d must not exceed 28 right-hand sides)");
    if (w > fit) return fail(h, GPSLAM_E_UNSUPPORTED, "loop closures in column passes: closures_per_pass is larger than fits (1 + landmarks * landmark_dim + closures_per_pass * d must not exceed 28 right-hand sides)");
    w = std::min(w, h->clo.n);
    const int P = (h->clo.n + w - 1) / w;
    if (P > 1) {
      if (h->clo.nc > kCloWideMax) return fail(h, GPSLAM_E_UNSUPPORTED, "too many loop closures: closures * d must not exceed 120");
      if (P > h->clo.max_passes) return fail(h, GPSLAM_E_UNSUPPORTED, "too many loop closures for max_passes column passes (set_closure_passes): closures / closures per pass exceeds it");
      passes = true;
    }
    h->clo.slice = w;
    h->clo.P = P;
  }
  h->R = 1 + h->nl + (passes ? h->clo.slice * d : h->clo.nc);
  h->fs.active = false;
  segmented = h->nl > 0 && (h->cfg.force_segmented == 1 || h->fs.split || 3 * b + h->R > 64 || h->R > kMaxRhs);
  if (h->fs.split) {
    if (!segmented) return fail(h, GPSLAM_E_INVALID, "a piece of a split chain (fs_set_split) needs landmarks: chains without them shard with nranks > 1");
    for (const std::vector<int> *v : {&h->fs.first_lm, &h->fs.last_lm})
      for (int l : *v) if (l < 0 || l >= h->L) return fail(h, GPSLAM_E_INVALID, "fs_set_split: landmark index out of range");
    h->fs.nb_top = 0;
  }
  if (h->clo.n > 0) {   // loop closures: d extra right-hand sides each, through the dense-border path of the chain solver
    if (!kIsF64) return fail(h, GPSLAM_E_UNSUPPORTED, "loop closures on an fp32 handle");
    if (sharded(h)) return fail(h, GPSLAM_E_UNSUPPORTED, "loop closures on a sharded handle");
    if (segmented) return fail(h, GPSLAM_E_UNSUPPORTED, "loop closures together with the segmented landmark elimination (too many landmark + closure columns for the dense border: 1 + landmarks * dim + closures * d <= 28)");
    if (h->R > kMaxRhs || 3 * b + h->R > 64)
      return fail(h, GPSLAM_E_UNSUPPORTED, "too many loop closures: 1 + landmarks * landmark_dim + closures * d must not exceed 28 right-hand sides");
  }
  if (any_robust(h)) {   // noiseModel::Robust: the fp64 factor kernels of one unsharded handle
    if (!kIsF64) return fail(h, GPSLAM_E_UNSUPPORTED, "robust noise models (set_meas_robust / set_between_pairs_robust) on an fp32 handle");
    if (sharded(h)) return fail(h, GPSLAM_E_UNSUPPORTED, "robust noise models (set_meas_robust / set_between_pairs_robust) on a sharded handle");
    if (h->fs.split) return fail(h, GPSLAM_E_UNSUPPORTED, "robust noise models (set_meas_robust / set_between_pairs_robust) on a piece of a split chain");
  }
  if (h->sg.count() > 0) {   // joint Gaussians on one state (fixedlag.hip): the fp64 factor kernel of one unsharded handle with the dense border
    if (!kIsF64) return fail(h, GPSLAM_E_UNSUPPORTED, "state Gaussians (add_state_gaussians) on an fp32 handle");
    if (sharded(h)) return fail(h, GPSLAM_E_UNSUPPORTED, "state Gaussians (add_state_gaussians) on a sharded handle");
    if (h->fs.split) return fail(h, GPSLAM_E_UNSUPPORTED, "state Gaussians (add_state_gaussians) on a piece of a split chain");
    if (segmented) return fail(h, GPSLAM_E_UNSUPPORTED, "state Gaussians (add_state_gaussians) together with the segmented landmark elimination");
    if (h->mf == ROT3_BIAS) return fail(h, GPSLAM_E_UNSUPPORTED, "state Gaussians (add_state_gaussians) on a GPSLAM_ROT3_BIAS handle (the pad coordinates of its velocity slot)");
  }
  if (h->bg.count() > 0) {   // joint Gaussians on one state and the landmarks (fixedlag.hip): as the state Gaussians, on the dense border
    if (!kIsF64) return fail(h, GPSLAM_E_UNSUPPORTED, "border Gaussians (add_border_gaussians) on an fp32 handle");
    if (sharded(h)) return fail(h, GPSLAM_E_UNSUPPORTED, "border Gaussians (add_border_gaussians) on a sharded handle");
    if (h->fs.split) return fail(h, GPSLAM_E_UNSUPPORTED, "border Gaussians (add_border_gaussians) on a piece of a split chain");
    if (segmented) return fail(h, GPSLAM_E_UNSUPPORTED, "border Gaussians (add_border_gaussians) together with the segmented landmark elimination");
    if (h->mf == ROT3_BIAS) return fail(h, GPSLAM_E_UNSUPPORTED, "border Gaussians (add_border_gaussians) on a GPSLAM_ROT3_BIAS handle (the pad coordinates of its velocity slot)");
    if (passes) return fail(h, GPSLAM_E_UNSUPPORTED, "border Gaussians (add_border_gaussians) together with loop closures in column passes (set_closure_passes): the final pass's right-hand sides are the closures' alone");
  }
  if (segmented) {
    if (sharded(h)) return fail(h, GPSLAM_E_UNSUPPORTED, "the segmented landmark elimination splits across GPUs through gpslam_hip_fs_set_split (pieces joined at shared cut states), not through nranks > 1");
    h->R = 1;   // no landmark columns inside the chain solver
  }
  return 0;
}

// Where every factor's rows sit in the two row tables, and what the record forms need to know about that placement
struct RowLayout {
  std::vector<int> rowptr, crowptr;                                        // N + 2 row pointers: full-width table, compact table
  std::vector<int> gp_row0, r_pri, r_vpri, r_sg, r_btw, r_ms[kNumMeasKinds];    // first row of every factor
  std::vector<int> gpidx, btwidx;          // N + 2 entries: the GP prior / between factor whose left state is s, or -1
  bool one_gp = true, one_btw = true;      // at most one GP prior / between factor per left state
  bool gp_rows_lead = true, btw_rows_trail = true;
};
bool index_by_left(const std::vector<int32_t> &left, int N, std::vector<int> &idx) {
  idx.assign(N + 2, -1);
  bool one = true;
  for (size_t f = 0; f < left.size(); f++) {
    if (idx[left[f]] >= 0) one = false;
    idx[left[f]] = (int)f;
  }
  return one;
}
// rows grouped by left state; inside a state: GP, pose prior, velocity prior, state Gaussian, between, measurements.  Pose priors and between
// factors are velocity-free: their rows go to the compact table.
void layout_rows(gpslam_hip_handle *h, RowLayout &lay) {
  const int N = h->N, d = h->d, b = h->b;
  std::vector<int> rows_in(N + 1, 0), crows_in(N + 1, 0);
  for (int32_t l : h->gp_left) rows_in[l] += b;
  for (int32_t i : h->vpri.idx) rows_in[i] += d;
  for (int32_t i : h->sg.idx) rows_in[i] += b;
  for (int32_t i : h->pri.idx) crows_in[i] += d;
  for (int32_t i : h->btw.idx) crows_in[i] += d;
  for (MeasSet &s : h->ms) for (int32_t i : s.idx) rows_in[i] += s.rows;
  lay.rowptr.assign(N + 2, 0);
  lay.crowptr.assign(N + 2, 0);
  for (int s = 0; s <= N; s++) { lay.rowptr[s + 1] = lay.rowptr[s] + rows_in[s]; lay.crowptr[s + 1] = lay.crowptr[s] + crows_in[s]; }
  h->M = lay.rowptr[N + 1];
  h->Mc = lay.crowptr[N + 1];
  std::vector<int> cursor(lay.rowptr.begin(), lay.rowptr.end() - 1), ccursor(lay.crowptr.begin(), lay.crowptr.end() - 1);
  auto place = [](std::vector<int> &cur, const std::vector<int32_t> &idx, int rows, std::vector<int> &row0) {
    row0.resize(idx.size());
    for (size_t f = 0; f < idx.size(); f++) { row0[f] = cur[idx[f]]; cur[idx[f]] += rows; }
  };
  place(cursor, h->gp_left, b, lay.gp_row0);
  place(ccursor, h->pri.idx, d, lay.r_pri);
  place(cursor, h->vpri.idx, d, lay.r_vpri);
  place(cursor, h->sg.idx, b, lay.r_sg);
  place(ccursor, h->btw.idx, d, lay.r_btw);
  for (int fk = 0; fk < kNumMeasKinds; fk++) place(cursor, h->ms[fk].idx, h->ms[fk].rows, lay.r_ms[fk]);
  // What the record decoders assume about this placement (k_assemble_ghost's `rp_s += B`, k_fused_level0's `p0 += B` / `q1 -= Dh`):
  // a state's GP-prior rows LEAD its range of the full-width table and its between factor's rows END its range of the compact
  // table.  True by the order of the calls above; checked here so that a change of that order turns the record paths off
  // (make_plan) instead of silently skipping or double-counting rows (ADVICE r4).
  for (size_t f = 0; f < h->gp_left.size(); f++) lay.gp_rows_lead = lay.gp_rows_lead && lay.gp_row0[f] == lay.rowptr[h->gp_left[f]];
  for (size_t f = 0; f < h->btw.idx.size(); f++) lay.btw_rows_trail = lay.btw_rows_trail && lay.r_btw[f] + d == lay.crowptr[h->btw.idx[f] + 1];
  lay.one_gp = index_by_left(h->gp_left, N, lay.gpidx);
  lay.one_btw = index_by_left(h->btw.idx, N, lay.btwidx);
}

// GP priors with more than one distinct Qc: the device-side arrays are ordered by Qc, one launch per group (host side only)
void group_gp_by_qc(gpslam_hip_handle *h) {
  const size_t F = h->gp_left.size();
  if (h->gp_q.size() != F) h->gp_q.assign(F, 0);
  h->gp_perm.resize(F);
  for (size_t f = 0; f < F; f++) h->gp_perm[f] = (int32_t)f;
  std::stable_sort(h->gp_perm.begin(), h->gp_perm.end(), [&](int32_t x, int32_t y) { return h->gp_q[x] < h->gp_q[y]; });
  h->gp_groups.clear();
  for (size_t k = 0; k < F; k++) {
    const int q = h->gp_q[h->gp_perm[k]];
    if (h->gp_groups.empty() || h->gp_groups[h->gp_groups.size() - 3] != q) { h->gp_groups.push_back(q); h->gp_groups.push_back((int32_t)k); h->gp_groups.push_back(0); }
    h->gp_groups.back()++;
  }
  if (h->gp_groups.size() == 3 && h->gp_groups[0] == 0) h->gp_groups.clear();   // the common case: everything shares set_qc's Qc
  // every prior added with its own Qc_model, all of them the same matrix (what the host classes and the GTSAM adapter
  // produce for a graph with one shared Qc): still ONE launch, and the structured records use that U (ADVICE r3)
  h->gp_single_q = (h->gp_groups.size() == 3 && h->gp_groups[0] > 0) ? h->gp_groups[0] : 0;
}

// every factor set and the row pointers to the device, the row tables sized; npart: partial sums the factor kernels of one pass leave
int upload_factors(gpslam_hip_handle *h, const RowLayout &lay, int &npart) {
  const int d = h->d, b = h->b;
  int rc;
  if ((rc = upload(h, h->rowptr, lay.rowptr))) return rc;
  {
    const size_t F = h->gp_left.size();
    std::vector<int32_t> pl(F); std::vector<double> pdt(F); std::vector<int> pr(F);
    for (size_t k = 0; k < F; k++) { pl[k] = h->gp_left[h->gp_perm[k]]; pdt[k] = h->gp_dt[h->gp_perm[k]]; pr[k] = lay.gp_row0[h->gp_perm[k]]; }
    if ((rc = upload(h, h->d_gp_left, pl))) return rc;
    if ((rc = upload(h, h->d_gp_dt, pdt))) return rc;
    if ((rc = upload(h, h->d_gp_row0, pr))) return rc;
  }
  if ((rc = upload_set(h, h->pri, lay.r_pri))) return rc;
  if ((rc = upload_set(h, h->vpri, lay.r_vpri))) return rc;
  if ((rc = upload_set(h, h->btw, lay.r_btw))) return rc;
  if ((rc = upload_set(h, h->lpri, std::vector<int>()))) return rc;
  if (h->clo.n > 0 && (rc = closures_upload(h))) return rc;
  if (h->sg.count() > 0 && (rc = state_gauss_upload(h, lay.r_sg))) return rc;
  if (kIsF64 && h->bg.count() > 0 && (rc = border_gauss_upload(h))) return rc;
  // (one k_gp launch per distinct Qc, each rounding its factor count up to whole blocks: at most one extra slot per group)
  npart = nblocks((int)h->gp_left.size(), 128) + gp_ngroups(h) + nblocks(h->pri.count(), 128) + nblocks(h->vpri.count(), 128) +
          nblocks(h->btw.count(), 128) + 1 + 256 + 1 + nblocks(h->sg.count(), 128) + 1;   // (+ 1: the loop closures' error; + 1: the border Gaussians')
  for (int fk = 0; fk < kNumMeasKinds; fk++) {
    MeasSet &s = h->ms[fk];
    if ((rc = upload(h, s.d_idx, s.idx))) return rc;
    if ((rc = upload(h, s.d_lm, s.lm))) return rc;
    if ((rc = upload(h, s.d_meas, s.meas))) return rc;
    if ((rc = upload(h, s.d_sig, s.sig))) return rc;
    if ((rc = upload(h, s.d_row0, lay.r_ms[fk]))) return rc;
    std::vector<double> coef((size_t)(s.interp ? s.count() : 0) * 4);
    for (int k = 0; k < (s.interp ? s.count() : 0); k++) interp_coef(s.dt[k], s.tau[k], &coef[4 * (size_t)k]);
    if ((rc = upload(h, s.d_coef, coef))) return rc;
    if ((rc = upload(h, s.d_aux, s.aux))) return rc;
    if ((rc = upload(h, s.d_aidx, s.aidx))) return rc;
    if ((rc = upload(h, s.d_sqi, s.sqi))) return rc;
    if ((rc = upload(h, s.d_rob, s.rob))) return rc;
    if (!s.rob.empty()) HIPCHK(s.d_w.reserve((size_t)s.count() * sizeof(RowT)));
    npart += nblocks(s.count(), 128);
  }
  const size_t Mrows = (size_t)std::max(h->M, 1);
  // one row of slack behind each table: the assembly kernels issue their row loads unconditionally from a clamped index,
  // and for a state WITHOUT rows (the chain's last state has no factor to its right) that index is rowptr[s] == M, one row
  // past the end (the value is never used).  Found in round 3 when a new buffer moved the tables to the end of a mapping.
  HIPCHK(h->rowLR.reserve((Mrows + 1) * 2 * b * sizeof(RowT)));
  HIPCHK(h->rowE.reserve((Mrows + 1) * sizeof(RowT)));
  HIPCHK(h->rowC.reserve((size_t)(std::max(h->Mc, 1) + 1) * b * sizeof(RowT)));
  HIPCHK(h->rowCE.reserve((size_t)(std::max(h->Mc, 1) + 1) * sizeof(RowT)));
  return upload(h, h->crowptr, lay.crowptr);
}

// landmark columns of the rows, the rows of each landmark (by left state), and -- dense border -- their chunked reduction;
// touch_lo / touch_hi: first / last state the factors of each landmark touch (what the segmented path cuts the chain by)
int build_landmark_border(gpslam_hip_handle *h, const RowLayout &lay, bool segmented, std::vector<int> &touch_lo, std::vector<int> &touch_hi) {
  int rc;
  h->nlmrows = 0;
  touch_lo.assign(h->L, -1);
  touch_hi.assign(h->L, -1);
  if (h->nl <= 0) return 0;
  const size_t Mrows = (size_t)std::max(h->M, 1);
  HIPCHK(h->rowM.reserve((Mrows + 1) * h->ld * sizeof(RowT)));
  HIPCHK(h->rowLm.reserve((Mrows + 1) * sizeof(int)));
  HIPCHK(hipMemsetAsync(h->rowM.p, 0, Mrows * h->ld * sizeof(RowT), h->stream));
  HIPCHK(hipMemsetAsync(h->rowLm.p, 0xFF, Mrows * sizeof(int), h->stream));  // -1: row touches no landmark
  std::vector<std::vector<std::pair<int, int>>> per_lm(h->L);              // (row, state)
  for (int fk = 0; fk < kNumMeasKinds; fk++) {
    MeasSet &s = h->ms[fk];
    if (!s.haslm) continue;
    for (int f = 0; f < s.count(); f++) {
      for (int r = 0; r < s.rows; r++) per_lm[s.lm[f]].push_back({lay.r_ms[fk][f] + r, s.idx[f]});
      int &lo = touch_lo[s.lm[f]], &hi = touch_hi[s.lm[f]];
      const int last = s.idx[f] + (s.two ? 1 : 0);
      lo = (lo < 0) ? s.idx[f] : std::min(lo, (int)s.idx[f]);
      hi = std::max(hi, last);
    }
  }
  std::vector<int> lmrow, lmstate, lmptr(h->L + 1, 0);
  for (int l = 0; l < h->L; l++) {
    // by left state (stable: equal states keep the order the factors were added in): the segmented path walks a
    // landmark's rows along the chain, and the dense path's summation order is then independent of the call order
    std::stable_sort(per_lm[l].begin(), per_lm[l].end(), [](const std::pair<int, int> &x, const std::pair<int, int> &y) { return x.second < y.second; });
    for (auto &pr : per_lm[l]) { lmrow.push_back(pr.first); lmstate.push_back(pr.second); }
    lmptr[l + 1] = (int)lmrow.size();
  }
  h->nlmrows = (int)lmrow.size();
  if (segmented) { h->fs.h_lmrow = lmrow; h->fs.h_lmstate = lmstate; h->fs.h_lmptr = lmptr; }
  if (!segmented) {   // chunks of at most kLmChunk consecutive rows of one landmark
    std::vector<int> clm, cj0, cj1, cptr(h->L + 1, 0);
    for (int l = 0; l < h->L; l++) {
      for (int j = lmptr[l]; j < lmptr[l + 1]; j += kLmChunk) {
        clm.push_back(l); cj0.push_back(j); cj1.push_back(std::min(j + kLmChunk, lmptr[l + 1]));
      }
      cptr[l + 1] = (int)clm.size();
    }
    h->nlmchunks = (int)clm.size();
    if ((rc = upload(h, h->lm_chunk_lm, clm))) return rc;
    if ((rc = upload(h, h->lm_chunk_j0, cj0))) return rc;
    if ((rc = upload(h, h->lm_chunk_j1, cj1))) return rc;
    if ((rc = upload(h, h->lm_chunk_ptr, cptr))) return rc;
    HIPCHK(h->lm_part.reserve((size_t)std::max(h->nlmchunks, 1) * 2 * h->ld * h->R * sizeof(Real)));
  }
  if ((rc = upload(h, h->lmrow, lmrow))) return rc;
  if ((rc = upload(h, h->lmrow_state, lmstate))) return rc;
  if ((rc = upload(h, h->lmrow_ptr, lmptr))) return rc;
  if (!segmented) {
    HIPCHK(h->lm_t.reserve((size_t)std::max(h->nlmrows, 1) * h->R * sizeof(Real)));
    HIPCHK(h->lm_S.reserve(((size_t)h->nl * h->R + h->nl) * sizeof(Real)));   // [S (nl x R) | gL (nl)]: one buffer, one all-reduce
  }
  HIPCHK(h->lm_dL.reserve((size_t)h->nl * sizeof(Real)));
  if (!h->lmk.p) return fail(h, GPSLAM_E_INVALID, "set_landmarks() before compile()");
  return 0;
}

// partial sums, gradient copies and the update vector of the optimiser loops
int size_workspace(gpslam_hip_handle *h, int npart) {
  const int N = h->N, b = h->b;
  npart = std::max(npart, std::max(nblocks(N, 128), 3 * nblocks(N * b, 256))) + 4200;   // (3 x: launch_dot3's three partial arrays)
  HIPCHK(h->partial.reserve((size_t)npart * sizeof(double)));   // the fp64 error pass of an fp32 handle uses it as well
  HIPCHK(h->partial2.reserve((size_t)(nblocks(N, 128) + 8) * sizeof(double)));
  h->defer.clear();
  HIPCHK(h->gsave.reserve((size_t)N * b * sizeof(Real)));
  HIPCHK(h->gsave2.reserve((size_t)(N + 1) * b * sizeof(Real)));   // (LM through the fused kernel: separator parts)
  HIPCHK(hipMemsetAsync(h->gsave2.p, 0, (size_t)(N + 1) * b * sizeof(Real), h->stream));
  HIPCHK(h->dvec.reserve((size_t)N * b * sizeof(Real)));
  return 0;
}

// Solver hierarchy: chunks of m0 states at level 0, m1 above.  Unsharded: a single-wave sequential top
// level of <= `top` blocks.  Sharded: reduce down to one block per rank (the rank separator).
// upper_chunk / top_blocks override the upper-level chunk length and the size of the sequential top level
// Level-0 chunk length: `slots` chunks run at once and a launch costs (rounds of slots) x (block steps per chunk);
// pick the length that minimises that product (1e5 Pose3 states on 256 CUs: 13 -> 7693 chunks, one round of 12 steps
// of the row-layout kernel; the column-layout kernel gets 25 -> 4000 chunks, one round of 24 steps).
int build_hierarchy(gpslam_hip_handle *h, const Plan &p) {
  const int N = h->N, b = h->b;
  int m0 = 16;
  if (h->cfg.chunk > 1) {
    m0 = h->cfg.chunk;
  } else {
    hipDeviceProp_t prop;
    const int cus = (hipGetDeviceProperties(&prop, h->cfg.device) == hipSuccess && prop.multiProcessorCount > 0)
                        ? prop.multiProcessorCount : 256;
    // column-layout kernel: one chunk per wave, 4 waves per SIMD; row-layout kernel: four chunks per wave, 2 waves per SIMD
    // (the fused kernel: four two-wave workgroups of four chunks per CU)
    const long slots = (long)cus * (p.fused() ? 16 : p.rows() ? 32 : 16);
    // rounds of resident chunks x block steps per chunk.  Round 3: a chunk of the row-layout kernels costs about three block
    // steps besides its own (the two leading images / the separator's record, the hand-over at the end), which the count of
    // steps alone ignored: at 1e6 states it chose chunks of 8 (31 rounds x 7 steps) where chunks of 32 are 9 % faster
    // (scripts/sweep_chunk.py: 3.86 -> 3.51 ms per iteration; fused level 0 2.11 -> 1.82 ms)
    const int overhead = p.rows() ? 3 : 0;
    long best = -1;
    for (int m = p.rows() ? 8 : 16; m <= 32; m++) {
      const long chunks = (N + m - 1) / m;
      const long cost = ((chunks + slots - 1) / slots) * (m - 1 + overhead);
      if (best < 0 || cost <= best) { best = cost; m0 = m; }   // ties: the longer chunk leaves fewer separators
    }
  }
  const int m1 = h->cfg.upper_chunk > 1 ? h->cfg.upper_chunk : 4;
  const int top = h->cfg.top_blocks > 0 ? h->cfg.top_blocks : 8;
  h->lv.clear();
  const size_t BS = (size_t)2 * b * b + (size_t)b * h->R, AS = (size_t)b * b + (size_t)b * h->R;
  int n = N;
  for (int l = 0;; l++) {
    Level v;
    v.n = n;
    v.m = (l == 0) ? m0 : (p.upper_cr ? kUpG : m1);
    // level 1 of a chain the row-layout level-0 kernels serve (four chunks per wave): groups of four, which
    // k_fused_level0 reduces in its own tail -- when there are enough separators for it to save a launch
    // (not on a sharded handle: the padding of the tail would sit between the last state and the next rank's separator)
    if (l == 1 && p.upper_cr && p.rows() && n > kUpG && !sharded(h)) v.m = 4;
    v.nch = nblocks(n, v.m);
    h->lv.push_back(std::move(v));
    if (n <= ((l >= 1 && p.upper_cr) ? kUpG : top)) break;
    n = h->lv.back().nch;
  }
  for (size_t l = 0; l < h->lv.size(); l++) {
    Level &v = h->lv[l];
    HIPCHK(v.blk.reserve((size_t)v.n * BS * sizeof(Real)));
    // + 1: solution of the neighbour rank's separator; + 64 values behind it: where the lanes of k_chunk_backward_rows that hold no
    // row store (its stores are unconditional)
    HIPCHK(v.x.reserve(((size_t)(v.n + 1) * b * h->R + 64) * sizeof(Real)));
    if (l > 0) {
      HIPCHK(v.add.reserve((size_t)(v.n + 1) * AS * sizeof(Real)));
      HIPCHK(hipMemsetAsync(v.add.p, 0, (size_t)(v.n + 1) * AS * sizeof(Real), h->stream));
    }
  }
  if (sharded(h)) {
    const int P = h->cfg.nranks;
    HIPCHK(h->halo_add.reserve(AS * sizeof(Real)));
    HIPCHK(h->iface_send.reserve((BS + AS) * sizeof(Real)));
    HIPCHK(h->iface_recv.reserve((size_t)P * (BS + AS) * sizeof(Real)));
    HIPCHK(h->top_blk.reserve((size_t)P * BS * sizeof(Real)));
    HIPCHK(h->top_x.reserve((size_t)(P + 1) * b * h->R * sizeof(Real)));
    HIPCHK(hipMemsetAsync(h->halo_add.p, 0, AS * sizeof(Real), h->stream));
    HIPCHK(hipMemsetAsync(h->iface_send.p, 0, (BS + AS) * sizeof(Real), h->stream));
    HIPCHK(hipMemsetAsync(h->iface_recv.p, 0, (size_t)P * (BS + AS) * sizeof(Real), h->stream));
    HIPCHK(hipMemsetAsync(h->top_x.p, 0, (size_t)(P + 1) * b * h->R * sizeof(Real), h->stream));
  }
  return 0;
}

// The plan (api_common.hpp: Plan) of the graph being compiled: every "does this form apply" is decided here, once.  Kernel selection
// is per handle and visible -- gpslam_hip_config_v2.plan (v1: reserved[6]) is a mask of GPSLAM_PLAN_* bits (the process-environment
// switches of rounds 2 / 3 are gone).  The fallback families a bit selects are the ones chains with landmark columns, pinned
// hierarchy shapes or wide borders need anyway; the bits keep them tested on plain chains.
// The chunk length follows from the level-0 family and the folds from the shape of the hierarchy, so the hierarchy is built here,
// between the two.
int make_plan(gpslam_hip_handle *h, const RowLayout &lay) {
  const int N = h->N, b = h->b;
  const int ngp = (int)h->gp_left.size();
  const int other = h->M - ngp * b;       // full-width rows besides the GP priors'
  Plan p;
  p.gp_rows_lead = lay.gp_rows_lead;
  p.btw_rows_trail = lay.btw_rows_trail;
  // a handful (a velocity prior or two) are fetched where they are used (k_fused_level0<2>, no ring); more than that -- interpolated
  // measurement factors, a dozen rows per state -- get a ring next to the records (<3>, round 4)
  p.odd_rows = other == 0 ? 0 : (other > 4 * b ? 2 : 1);
  // GP priors as records: fp64, at most one per left state, one Qc (the handle's, or the same one on every prior), their rows
  // leading the state's range; GPSLAM_PLAN_GP_ROWS keeps plain Jacobian rows (the rows path of every chain)
  const bool rec_ok = kIsF64 && lay.one_gp && ngp > 0 && p.gp_rows_lead && (gp_ngroups(h) == 0 || h->gp_single_q > 0) && !plan_bit(h, GPSLAM_PLAN_GP_ROWS);
  const bool d3 = h->mf == POSE2 || h->mf == ROT3 || h->mf == LINEAR3;   // block size 6
  p.pure6 = rec_ok && d3 && other <= 4 * b;
  // k_chunk_forward_rows covers every block size with a single right-hand side (round 3: 6 and 4 as well;
  // GPSLAM_PLAN_COLUMN_LEVEL0 keeps the column-layout kernel)
  const bool rows = !plan_bit(h, GPSLAM_PLAN_COLUMN_LEVEL0) && (b == 12 || b == 6 || b == 4) && h->R == 1;
  // k_fused_level0 (assembly inside the level-0 elimination): chains of block size 12 or 6 (round 3: SE(2), SO(3), 3-D linear)
  // without landmark columns (GPSLAM_PLAN_UNFUSED_LEVEL0 keeps k_assemble_ghost + k_chunk_forward_rows); on a sharded handle
  // the rows of the last local state carry their R^T R to the next rank inside the addend the last chunk sends upward,
  // which is what k_assemble_ghost's halo addend used to hold.
  // Block size 6: a block step is a fifth of the SE(3) step's arithmetic but keeps its LDS hand-overs and row-ring round trips, so
  // the fused kernel is latency bound -- it wins while the launch it saves and the chip's ramp matter (1e5 states: C2 0.209 ->
  // 0.177 ms, C5 SO(3) 0.330 -> 0.296) and loses to the two streaming kernels at scale (1e6: C2 1.35 -> 1.57 ms).  Hence the
  // size rule.
  // Round 4: a block-size-6 chain whose full-width rows are (all but a handful) GP priors that travel as d = 3 records (pure6) has
  // next to nothing left to fetch per block step -- fused at every size (1e6 states: C2 0.99 -> 0.94 ms, 3e5: 0.334 -> 0.321);
  // with measurement rows in the ring the rule stands (C5 SO(3) + attitude at 1e6: 1.74 unfused, 1.86 fused).
  const bool b6 = b == 6 && (N <= 131072 || p.pure6);
  const bool fused = (b == 12 || b6) && rows && h->nl == 0 && !plan_bit(h, GPSLAM_PLAN_UNFUSED_LEVEL0);   // (fp32 rows are widened as the assembly wave reads them)
  p.level0 = fused ? Level0::Fused : (rows ? Level0::Rows : Level0::Column);
  // The levels above level 0 as LDS-resident cyclic reduction, 32 blocks per workgroup and launch (upper.hip): chains
  // without landmark columns (sharded or not), unless the caller pinned the old hierarchy's shape (upper_chunk / top_blocks).
  // GPSLAM_PLAN_LEVELS_OF_FOUR keeps one launch per level of chunks of four.
  p.upper_cr = !plan_bit(h, GPSLAM_PLAN_LEVELS_OF_FOUR) && h->R == 1 && h->cfg.upper_chunk <= 1 && h->cfg.top_blocks <= 0;
  int rc;
  if ((rc = build_hierarchy(h, p))) return rc;
  // level 1 as groups of four (build_hierarchy): the fused kernel's tail reduces them, and where the groups are exactly the waves
  // of the row-layout back-substitution (launch_backward) that kernel solves them
  p.tail_fold = p.upper_cr && h->lv.size() >= 3 && h->lv[1].m == 4;
  p.fold_tail_bwd = kIsF64 && p.tail_fold && !sharded(h) && h->R == 1 && rows && h->lv[1].n == h->lv[0].nch;
  // SE(3): body-velocity chains under the fused kernel; block size 6: SE(2), SO(3) and 3-D linear chains (any other factors)
  if (rec_ok && fused && h->mf == POSE3 && !h->vw) p.gp_rec = GpForm::Se3Rec;
  else if (rec_ok && d3) p.gp_rec = GpForm::D3Rec;
  const bool se3 = p.gp_rec == GpForm::Se3Rec;
  // (chains with other full-width rows besides the GP priors' run k_fused_level0<2>, which keeps compact rows)
  p.btw_rec = se3 && lay.one_btw && p.btw_rows_trail && h->btw.count() > 0 && other == 0;
  {   // the retraction folded into the next K1 inside run_gn (PendUpd): record chains (SE(3), and the d = 3 manifolds: config 2) on
      // one unsharded handle whose every state but the last is the left state of exactly one GP prior (the owner that writes it
      // back), one k_lin launch (a single Qc)
    bool ok = p.gp_rec != GpForm::Rows && h->lv.size() >= 2 && !sharded(h) && h->nl == 0 && h->clo.n == 0 && gp_ngroups(h) <= 1 &&
              ngp == N - 1 && N >= 2;      // (lv.size() >= 2: the fused level 0, whose K1 writes the records, runs)
    // measurement factors: on SE(3) record chains k_meas runs BEHIND k_lin on the same stream (it reads the interval's record) and
    // so behind the buffer swap -- it sees the updated states; on the d = 3 chains it reads nothing k_lin writes (a launch that
    // forks puts it on the second stream) -- the kinds that read two states (the interpolated ones) apply the pending update themselves
    // from the old buffer
    for (int fk = 0; fk < kNumMeasKinds && ok; fk++) ok = h->ms[fk].count() == 0 || se3 || h->ms[fk].two;
    for (int f = 0; f < ngp && ok; f++) ok = h->gp_left[f] < N - 1;     // (one per left state: rec_ok)
    ok = ok && h->sg.count() == 0;      // (the state Gaussians' kernel reads the stored states: it applies no pending update)
    p.fold_retract = ok && !plan_bit(h, GPSLAM_PLAN_SEPARATE_RETRACT);
  }
  {   // interpolated measurement rows as 16-double lines next to the records (k_fused_level0<4>, kernels.hpp kIRow*): every
      // full-width row that is not a GP prior's belongs to an interpolated GPS factor on an interval with a GP prior (whose
      // record holds X, J and F of that interval); no landmarks (fused), no velocity priors
    const MeasSet &g = h->ms[FK_INTERP_GPS];
    // (a robust GPS factor needs |e| over its three rows before any of them is final: the row form through k_meas, as GPSLAM_PLAN_MEAS_ROWS)
    bool ok = se3 && !plan_bit(h, GPSLAM_PLAN_MEAS_ROWS) && g.rob.empty() && h->vpri.count() == 0 && h->sg.count() == 0 && g.count() > 0;
    for (int fk = 0; fk < kNumMeasKinds && ok; fk++) ok = (fk == FK_INTERP_GPS) || h->ms[fk].count() == 0;
    for (size_t f = 0; f < g.idx.size() && ok; f++) ok = lay.gpidx[g.idx[f]] >= 0;
    p.lines = ok;
  }
  h->plan = p;
  return 0;
}

// one record more than there are factors, all zeros (what the assembly wave reads for a state without a GP prior), and the U
// the records are whitened with
int alloc_gp_records(gpslam_hip_handle *h, int len) {
  const size_t F = h->gp_left.size();
  HIPCHK(h->gps.reserve((F + 1) * (size_t)len * sizeof(Real)));
  HIPCHK(hipMemsetAsync(static_cast<char *>(h->gps.p) + F * (size_t)len * sizeof(Real), 0, len * sizeof(Real), h->stream));
  h->dU_version = -1;
  return refresh_dU(h);
}
// the buffers and index tables of the forms the plan asks for
int alloc_records(gpslam_hip_handle *h, const RowLayout &lay) {
  const Plan &p = h->plan;
  const int N = h->N, b = h->b;
  int rc;
  if (p.fused() && !h->simd_cnt.p) {
    HIPCHK(h->simd_cnt.reserve(8192 * sizeof(int)));
    HIPCHK(hipMemsetAsync(h->simd_cnt.p, 0, 8192 * sizeof(int), h->stream));
  }
  const std::vector<int> none(N + 2, -1);
  if ((rc = upload(h, h->gpidx, p.gp_rec != GpForm::Rows ? lay.gpidx : none))) return rc;
  if (p.gp_rec == GpForm::D3Rec && (rc = alloc_gp_records(h, kGp3Len))) return rc;
  if ((rc = upload(h, h->btwidx, p.btw_rec ? lay.btwidx : none))) return rc;
  if (p.btw_rec) {
    HIPCHK(h->brec.reserve(((size_t)h->btw.count() + 1) * kBtwLen * sizeof(Real)));
    HIPCHK(hipMemsetAsync(static_cast<char *>(h->brec.p) + (size_t)h->btw.count() * kBtwLen * sizeof(Real), 0, kBtwLen * sizeof(Real), h->stream));
  }
  if (p.gp_rec == GpForm::Se3Rec && (rc = alloc_gp_records(h, kGpsLen))) return rc;
  h->defer.clear();
  if (p.fold_retract) {   // the second state buffer: here, not inside the first run's second iteration (a hipMalloc in a timed region)
    HIPCHK(h->pose_bak.reserve((size_t)h->pd * h->stride * sizeof(double)));
    HIPCHK(h->vel_bak.reserve((size_t)h->d * h->stride * sizeof(double)));
  }
  if (p.lines) {
    const MeasSet &g = h->ms[FK_INTERP_GPS];
    std::vector<int> irowptr(N + 2, 0), irow0(g.idx.size());
    for (int s = 0; s <= N; s++) irowptr[s + 1] = irowptr[s] + (lay.rowptr[s + 1] - lay.rowptr[s]) - (lay.gpidx[s] >= 0 ? b : 0);
    // (the GP prior's rows lead a state's range of the full-width table -- gp_rows_lead, part of the record forms -- so a
    //  measurement row keeps its place among the state's other rows)
    for (size_t f = 0; f < g.idx.size(); f++) irow0[f] = irowptr[g.idx[f]] + (lay.r_ms[FK_INTERP_GPS][f] - lay.rowptr[g.idx[f]] - b);
    if ((rc = upload(h, h->irowptr, irowptr))) return rc;
    if ((rc = upload(h, h->ms[FK_INTERP_GPS].d_irow0, irow0))) return rc;
    HIPCHK(h->rowI.reserve(((size_t)irowptr[N + 1] + 1) * kIRowLen * sizeof(Real)));
  }
  return 0;
}

int gpslam_hip_compile(gpslam_hip_handle *h) {
  if (!h || h->N <= 0) return GPSLAM_E_INVALID;
  (void)hipSetDevice(h->cfg.device);
  int rc, npart = 0;
  bool segmented = false;
  RowLayout lay;
  std::vector<int> touch_lo, touch_hi;
  if ((rc = check_stored_indices(h))) return rc;
  if ((rc = choose_landmark_path(h, segmented))) return rc;
  layout_rows(h, lay);
  group_gp_by_qc(h);
  if ((rc = upload_factors(h, lay, npart))) return rc;
  if ((rc = build_landmark_border(h, lay, segmented, touch_lo, touch_hi))) return rc;
  if ((rc = size_workspace(h, npart))) return rc;
  if ((rc = make_plan(h, lay))) return rc;          // (builds the solver hierarchy on its way)
  if ((rc = alloc_records(h, lay))) return rc;
  if (segmented && (rc = fs_build(h, touch_lo, touch_hi))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  h->compiled = true;
  return 0;
}

int gpslam_hip_linearize_gp(gpslam_hip_handle *h, double *errors, double *jacobians) {
  if (!kIsF64) return impl64::gpslam_hip_linearize_gp(h, errors, jacobians);   // the inspection API answers in fp64
  int rc = need_local(h);
  if (rc) return rc;
  if (!errors) return GPSLAM_E_INVALID;
  const int F = (int)h->gp_left.size(), b = h->b, d = h->d;
  if (F == 0) return 0;
  HIPCHK(h->api_e.reserve((size_t)F * b * sizeof(RowT)));
  if (jacobians) HIPCHK(h->api_H.reserve((size_t)F * 4 * b * d * sizeof(RowT)));
  // (unwhitened values do not depend on Qc: one launch over the device-side order, whatever the groups)
  GpArgs<RowT> a = gp_args(h, LaunchMode{}, nullptr);
  a.rowLR = nullptr; a.rowE = nullptr;
  a.out_e = h->api_e.as<RowT>(); a.out_H = jacobians ? h->api_H.as<RowT>() : nullptr;
  dispatch_mf(h->mf, [&](auto tag) {
    constexpr int MF = decltype(tag)::value;
    k_gp<RowT, MF, 2><<<dim3(nblocks(F, 128)), dim3(128), 0, h->stream>>>(a);
  });
  HIPCHK(hipGetLastError());
  const bool permuted = gp_ngroups(h) > 1;
  std::vector<double> te(permuted ? (size_t)F * b : 0), tH((permuted && jacobians) ? (size_t)F * 4 * b * d : 0);
  HIPCHK(hipMemcpyAsync(permuted ? te.data() : errors, h->api_e.p, (size_t)F * b * sizeof(Real), hipMemcpyDeviceToHost, h->stream));
  if (jacobians)
    HIPCHK(hipMemcpyAsync(permuted ? tH.data() : jacobians, h->api_H.p, (size_t)F * 4 * b * d * sizeof(Real), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (permuted) {   // back to the order the factors were added in
    for (int k = 0; k < F; k++) {
      const size_t o = (size_t)h->gp_perm[k];
      std::memcpy(errors + o * b, &te[(size_t)k * b], sizeof(double) * b);
      if (jacobians) std::memcpy(jacobians + o * 4 * b * d, &tH[(size_t)k * 4 * b * d], sizeof(double) * 4 * b * d);
    }
  }
  return F;
}

// k_meas's inspection mode on factors first .. first + count - 1 of one kind, in the order they were added: the unwhitened
// evaluateError() values into out_e (count x rows) and [H1 H2 | H3 H4 | H5 (3, zero padded)] per row into out_J, both on the device
// and of this namespace's row precision.  Writes them and `partial`, nothing else; no synchronisation
int launch_meas_inspect(gpslam_hip_handle *h, int kind, int first, int count, void *out_e, void *out_J) {
  MeasSet &s = h->ms[kind];
  if (first < 0 || count <= 0 || first + count > s.count() || !out_e || !out_J) return GPSLAM_E_INVALID;
  // no row tables: on an fp32 handle (this is impl64 answering for it) they hold floats, and a later solve must not find
  // this call's rows in them either way (ADVICE r3).  (a.rob stays null: evaluateError knows no noise model)
  MeasArgs<RowT> a = meas_args(h, kind);
  const size_t o = (size_t)first;
  a.count = count;
  a.idx += o; a.row0 += o;
  if (a.lm) a.lm += o;
  a.meas += o * s.mw; a.sig += o * s.rows;
  if (a.coef) a.coef += o * 4;
  if (a.aidx) a.aidx += o;
  if (a.sqi) a.sqi += o * s.rows * s.rows;
  a.partial = h->partial.as<RowT>();
  a.out_e = static_cast<RowT *>(out_e); a.out_J = static_cast<RowT *>(out_J);
  dispatch_mf(h->mf, [&](auto tag) {
    constexpr int MF = decltype(tag)::value;
    dispatch_fk(kind, [&](auto ftag) {
      constexpr int FK = decltype(ftag)::value;
      k_meas<RowT, MF, FK, true><<<dim3(nblocks(count, 128)), dim3(128), 0, h->stream>>>(a);
    });
  });
  HIPCHK(hipGetLastError());
  return 0;
}

// unwhitened evaluateError + H1..H5 of every measurement factor of one kind, in the order they were added
int gpslam_hip_linearize_meas(gpslam_hip_handle *h, int32_t kind, double *errors, double *jacobians) {
  if (!kIsF64) return impl64::gpslam_hip_linearize_meas(h, kind, errors, jacobians);   // the inspection API answers in fp64
  int rc = need_local(h);
  if (rc) return rc;
  if (kind < 0 || kind >= kNumMeasKinds || !errors) return GPSLAM_E_INVALID;
  MeasSet &s = h->ms[kind];
  const int F = s.count(), b = h->b, W = 2 * b + 3;
  if (F == 0) return 0;
  HIPCHK(h->api_e.reserve((size_t)F * s.rows * sizeof(RowT)));
  HIPCHK(h->api_H.reserve((size_t)F * s.rows * W * sizeof(RowT)));
  if ((rc = launch_meas_inspect(h, kind, 0, F, h->api_e.p, h->api_H.p))) return rc;
  HIPCHK(hipMemcpyAsync(errors, h->api_e.p, (size_t)F * s.rows * sizeof(RowT), hipMemcpyDeviceToHost, h->stream));
  if (jacobians) HIPCHK(hipMemcpyAsync(jacobians, h->api_H.p, (size_t)F * s.rows * W * sizeof(RowT), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return F;
}

// noiseModel::Robust: the weights w(r) of the measurement factors of one kind / of the closures at the current states, in the order
// they were added -- one error-only pass with MeasArgs::out_w / CloArgs::out_w set; factors without a loss report 1
int gpslam_hip_get_meas_weights(gpslam_hip_handle *h, int32_t kind, double *w) {
  int rc = need_local(h);
  if (rc) return rc;
  if (kind < 0 || kind >= kNumMeasKinds || !w) return GPSLAM_E_INVALID;
  MeasSet &s = h->ms[kind];
  const int F = s.count();
  if (s.rob.empty()) { for (int f = 0; f < F; f++) w[f] = 1.0; return F; }
  LaunchMode m;
  m.weights = true;
  if ((rc = launch_factors(h, m, 1, 1))) return rc;
  std::vector<RowT> t((size_t)F);
  HIPCHK(hipMemcpyAsync(t.data(), s.d_w.p, (size_t)F * sizeof(RowT), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int f = 0; f < F; f++) w[f] = (double)t[f];
  return F;
}
int gpslam_hip_get_between_pairs_weights(gpslam_hip_handle *h, double *w) {
  int rc = need_local(h);
  if (rc) return rc;
  if (!w) return GPSLAM_E_INVALID;
  const int F = h->clo.n;
  if (h->clo.rob.empty()) { for (int f = 0; f < F; f++) w[f] = 1.0; return F; }
  LaunchMode m;
  m.weights = true;
  if ((rc = launch_factors(h, m, 1, 1))) return rc;
  HIPCHK(hipMemcpyAsync(w, h->clo.w.p, (size_t)F * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return F;
}

int gpslam_hip_normal_equations(gpslam_hip_handle *h, double *D, double *O, double *g, double *B) {
  int rc = need_local(h);
  if (rc) return rc;
  if (B && h->fs.active) return fail(h, GPSLAM_E_UNSUPPORTED, "the dense landmark coupling B does not exist on the segmented landmark path");
  if ((rc = launch_factors(h, LaunchMode{}, 0, 0))) return rc;
  if ((rc = launch_assemble(h, LaunchMode{}, false))) return rc;
  const int N = h->N, b = h->b, R = h->R;
  const size_t BS = (size_t)2 * b * b + (size_t)b * R;
  std::vector<Real> blk((size_t)N * BS);
  HIPCHK(hipMemcpyAsync(blk.data(), h->lv[0].blk.p, blk.size() * sizeof(Real), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int s = 0; s < N; s++) {
    const Real *p = blk.data() + (size_t)s * BS;
    if (D) for (int k = 0; k < b * b; k++) D[(size_t)s * b * b + k] = p[k];
    if (O) for (int k = 0; k < b * b; k++) O[(size_t)s * b * b + k] = p[b * b + k];
    if (g) for (int k = 0; k < b; k++) g[(size_t)s * b + k] = p[2 * b * b + k];
    if (B && h->nl > 0)      // (the landmark columns; loop-closure columns behind them are not part of B)
      for (int k = 0; k < b; k++)
        for (int r = 1; r <= h->nl; r++) B[((size_t)s * b + k) * h->nl + (r - 1)] = p[2 * b * b + r * b + k];
  }
  return 0;
}

// whitened Jacobian rows of the current linearisation, in row-table order (rows grouped by left state; inside a
// state: GP priors, pose priors, velocity priors, between, then the measurement kinds in FKind order)
int gpslam_hip_get_rows(gpslam_hip_handle *h, int32_t *n_rows, double *rowLR, double *rowE, double *rowM, int32_t *rowLm) {
  int rc = need_local(h);
  if (rc) return rc;
  // the M rows of the full-width table, then the Mc compact rows (pose priors, between factors) expanded to full width
  const size_t M = (size_t)h->M, Mc = (size_t)h->Mc, b = (size_t)h->b, d = (size_t)h->d;
  if (n_rows) *n_rows = (int32_t)(M + Mc);
  if (!rowLR && !rowE && !rowM && !rowLm) return 0;
  LaunchMode m;
  m.d3_rows = true;                         // the table itself is wanted: no structured records
  if ((rc = launch_factors(h, m, 0, 0))) return rc;
  if (M + Mc == 0) return 0;
  std::vector<RowT> tLR(M * 2 * b), tE(M), tM(h->nl > 0 ? M * h->ld : 0), cLR(Mc * b), cE(Mc);
  if (M > 0) {
    HIPCHK(hipMemcpyAsync(tLR.data(), h->rowLR.p, tLR.size() * sizeof(RowT), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(tE.data(), h->rowE.p, tE.size() * sizeof(RowT), hipMemcpyDeviceToHost, h->stream));
    if (h->nl > 0) {
      HIPCHK(hipMemcpyAsync(tM.data(), h->rowM.p, tM.size() * sizeof(RowT), hipMemcpyDeviceToHost, h->stream));
      if (rowLm) HIPCHK(hipMemcpyAsync(rowLm, h->rowLm.p, M * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
  }
  if (Mc > 0) {
    HIPCHK(hipMemcpyAsync(cLR.data(), h->rowC.p, Mc * b * sizeof(RowT), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cE.data(), h->rowCE.p, Mc * sizeof(RowT), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  if (rowLR) for (size_t k = 0; k < tLR.size(); k++) rowLR[k] = (double)tLR[k];
  if (rowE) for (size_t k = 0; k < tE.size(); k++) rowE[k] = (double)tE[k];
  if (rowM) for (size_t k = 0; k < tM.size(); k++) rowM[k] = (double)tM[k];
  for (size_t r = 0; r < Mc; r++) {
    if (rowLR) {
      double *dst = rowLR + (M + r) * 2 * b;
      for (size_t k = 0; k < 2 * b; k++) dst[k] = 0.0;
      for (size_t k = 0; k < d; k++) { dst[k] = cLR[r * b + k]; dst[b + k] = cLR[r * b + d + k]; }
    }
    if (rowE) rowE[M + r] = cE[r];
    if (rowM) for (int q = 0; q < h->ld; q++) rowM[(M + r) * h->ld + q] = 0.0;
    if (rowLm) rowLm[M + r] = -1;
  }
  return 0;
}

int gpslam_hip_block_tridiag_solve(gpslam_hip_handle *h, int32_t N, const double *D, const double *O,
                                   const double *g, double *x) {
  int rc = need_local(h);
  if (rc) return rc;
  if (N != h->N || h->R != 1 || sharded(h) || !D || !O || !g || !x) return GPSLAM_E_INVALID;
  const int b = h->b;
  const size_t BS = (size_t)2 * b * b + b;
  std::vector<Real> blk((size_t)N * BS);
  for (int s = 0; s < N; s++) {
    Real *p = blk.data() + (size_t)s * BS;
    for (int k = 0; k < b * b; k++) { p[k] = D[(size_t)s * b * b + k]; p[b * b + k] = O[(size_t)s * b * b + k]; }
    for (int k = 0; k < b; k++) p[2 * b * b + k] = g[(size_t)s * b + k];
  }
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  HIPCHK(hipMemcpyAsync(h->lv[0].blk.p, blk.data(), blk.size() * sizeof(Real), hipMemcpyHostToDevice, h->stream));
  if ((rc = launch_solve(h, LaunchMode{}, 0.0))) return rc;
  std::vector<Real> xs((size_t)N * b);
  int flag = 0;
  HIPCHK(hipMemcpyAsync(xs.data(), h->lv[0].x.p, xs.size() * sizeof(Real), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&flag, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < xs.size(); i++) x[i] = xs[i];
  return flag ? fail(h, GPSLAM_E_NOT_SPD, "non-positive pivot") : 0;
}

int gpslam_hip_time_kernel(gpslam_hip_handle *h, int32_t which, int32_t reps, double *avg_ms) {
  int rc = need_local(h);
  if (rc) return rc;
  if (reps <= 0 || !avg_ms || which < 0 || which > 4 || sharded(h)) return GPSLAM_E_INVALID;
  double total = 0.0;
  // (every kernel is timed in the form an iteration runs it -- the launch helpers build the arguments; the SE(3) records belong to
  //  K1 and the fused elimination alone)
  LaunchMode m = level0_mode(h);
  m.se3_rec = m.se3_rec && (which == 0 || which == 2);
  for (int r = 0; r < reps; r++) {
    // bring the inputs of the timed kernel into their real state (untimed)
    if (which >= 1 && (rc = launch_factors(h, m, 0, 0))) return rc;
    if (which >= 2 && (rc = launch_assemble(h, m, false))) return rc;
    HIPCHK(hipEventRecord(h->ev[0], h->stream));
    if (which == 0) {
      GpArgs<RowT> a = gp_args(h, m, h->partial.as<RowT>(), false, gp_ngroups(h) >= 1 ? 0 : -1);   // (several Qc: the first group)
      const int nb = nblocks(a.count, 128);
      dispatch_mf(h->mf, [&](auto tag) {
        constexpr int MF = decltype(tag)::value;
        launch_gp_rows<MF>(h, a, nb);
      });
    } else if (which == 1) {
      if (m.fused) { *avg_ms = 0.0; return 0; }   // no such launch: see the header
      if ((rc = launch_assemble(h, m, false))) return rc;
    } else if (which == 2 || which == 3) {
      int grid;
      const FwdArgs<Real> a = fwd_args(h, m, 0, 0.0, grid);
      if ((rc = launch_fwd(h, m, a, grid))) return rc;
      if (which == 3) {  // time the level-0 back-substitution instead (separator solutions = whatever lv[1].x holds)
        HIPCHK(hipEventRecord(h->ev[0], h->stream));
        const BwdArgs<Real> bw = bwd_args(h, 0, nullptr, grid);
        launch_bwd(h, bw, grid);
      }
    } else {
      HIPCHK(hipMemsetAsync(h->lv[0].x.p, 0, (size_t)h->N * h->b * h->R * sizeof(Real), h->stream));
      HIPCHK(hipEventRecord(h->ev[0], h->stream));
      launch_retract_k(h);
    }
    HIPCHK(hipEventRecord(h->ev[1], h->stream));
    HIPCHK(hipEventSynchronize(h->ev[1]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    total += ms;
  }
  *avg_ms = total / reps;
  return 0;
}
