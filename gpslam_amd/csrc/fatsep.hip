// fatsep.hip -- the launches of the segmented landmark elimination (fatsep.hpp: BASELINE config 4, segments + fat separators), and
// compile()'s plan for it.  The one unit that includes fatsep.hpp, so every k_fs_* / k_fat_* kernel is compiled here, once per type of
// the Jacobian row tables: the solver's own numbers are double on every handle, and the rows' type is chosen once per call from the
// handle's precision (dispatch_row).  api_common.hpp declares the entry points and says where each one stands in an iteration.
#include "api_common.hpp"
#include "fatsep.hpp"

namespace {

typedef double Real;   // normal equations and solver: double whatever the rows are

// ---- row-type dispatch: call f(RowTag<double or float>{}) for the handle's precision
template <typename T> struct RowTag { typedef T type; };
template <typename F> int dispatch_row(const gpslam_hip_handle *h, F &&f) {
  return h->cfg.precision == GPSLAM_FP32 ? f(RowTag<float>{}) : f(RowTag<double>{});
}

// ---- dynamic LDS of each kernel that takes some, by the size it serves: used by its launch and by its attribute (fs_build).
// k_fs_sweep_syrk's is fatsep.hpp's fs_fused_smem
inline size_t fat_elim_mfma_lds(int NB) { return ((size_t)NB * (NB + 1) + (size_t)NB * (2 * NB + 1)) * sizeof(Real); }   // the factor + [H | H | g]
inline size_t fat_elim_wide_lds(int NB) { return ((size_t)NB * (NB + 1) + (size_t)NB * fat_wide_panel((int)sizeof(Real), NB)) * sizeof(Real); }
inline size_t fat_top_lds(int NB) { return ((size_t)NB * (NB + 1) + (size_t)NB) * sizeof(Real); }
inline size_t fat_back_w4_lds(int NB) { return ((size_t)NB * (NB + 1) + 3 * (size_t)NB) * sizeof(Real); }   // one operand + vectors
inline size_t fs_syrk_lds(int ncm) { return (size_t)2 * 24 * fs_lds_stride(ncm) * sizeof(Real); }   // 68 KB at NCM = 144

template <typename RowT> FsArgs<Real, RowT> fs_args(gpslam_hip_handle *h, double lambda) {
  FatSepPlan &p = h->fs;
  FsArgs<Real, RowT> a;
  a.N = h->N; a.B = h->b; a.ld = h->ld; a.L = h->L; a.K = p.K; a.NB = p.NB; a.NC = p.NC; a.NCP = p.NCP;
  a.BS = 2 * h->b * h->b + h->b;
  a.cuts = p.d_cuts.as<int>(); a.segid = p.d_segid.as<int>();
  a.fat_lm_ptr = p.d_fat_lm_ptr.as<int>(); a.fat_lm = p.d_fat_lm.as<int>();
  a.lm_fat = p.d_lm_fat.as<int>(); a.lm_slot = p.d_lm_slot.as<int>();
  a.lmrow_ptr = h->lmrow_ptr.as<int>(); a.lmrow = h->lmrow.as<int>(); a.lmrow_state = h->lmrow_state.as<int>();
  a.lmpri_ptr = p.d_lmpri_ptr.as<int>(); a.lmpri = p.d_lmpri.as<int>();
  a.lg_ptr = p.d_lg_ptr.as<int>(); a.lg_state = p.d_lg_state.as<int>(); a.lg_mptr = p.d_lg_mptr.as<int>(); a.lg_m = p.d_lg_m.as<int>();
  a.ngroups = p.ngroups; a.Gev = p.Gev.as<Real>();
  a.fa_ptr = p.d_fa_ptr.as<int>(); a.fa_it = p.d_fa_it.as<int>(); a.fb_ptr = p.d_fb_ptr.as<int>(); a.fb_it = p.d_fb_it.as<int>();
  a.fc_ptr = p.d_fc_ptr.as<int>(); a.fc_it = p.d_fc_it.as<int>();
  a.lmMM = p.lmMM.as<Real>();
  a.sc_base = p.d_sc_base.as<int>(); a.sc_ptr = p.d_sc_ptr.as<int>(); a.se_pk = p.d_se_pk.as<int>(); a.se_src = p.d_se_src.as<int>();
  a.pri_meas = h->lpri.d_meas.as<double>(); a.pri_sig = h->lpri.d_sig.as<double>();
  a.lmk = h->lmk.as<double>();
  a.rowptr = h->rowptr.as<int>(); a.rowLm = h->rowLm.as<int>();
  a.rowLR = h->rowLR.as<RowT>(); a.rowE = h->rowE.as<RowT>(); a.rowM = h->rowM.as<RowT>();
  a.blk = h->lv[0].blk.as<Real>();
  a.fac = p.fac.as<Real>(); a.Y = p.Y.as<Real>(); a.Aseg = p.Aseg.as<Real>();
  a.Dfat = p.Dfat.as<Real>(); a.link = p.link.as<Real>(); a.gfat = p.gfat.as<Real>(); a.Qbuf = p.Qbuf.as<Real>();
  a.S1 = p.S1.as<Real>(); a.S2 = p.S2.as<Real>(); a.sv = p.sv.as<Real>(); a.xfat = p.xfat.as<Real>();
  a.gL = h->lm_gL.as<Real>(); a.dL = h->lm_dL.as<Real>();
  a.x = h->lv[0].x.as<Real>(); a.rhs = p.rhs.as<Real>();
  a.lambda = (Real)lambda; a.flag = h->flag.as<int>();
  a.last_fat_shared = (p.split && p.rank < p.nranks - 1) ? 1 : 0;
  return a;
}

// a chain split across GPUs: the top system of the shared fat separators (P + 1 blocks of nb_top), solved redundantly by every
// piece with the very kernels of the cyclic reduction
template <typename RowT> FsArgs<Real, RowT> fs_top_args(gpslam_hip_handle *h) {
  FatSepPlan &p = h->fs;
  FsArgs<Real, RowT> t = fs_args<RowT>(h, 0.0);
  t.K = p.nranks + 1; t.NB = p.nb_top;
  t.Dfat = p.tD.as<Real>(); t.link = p.tlink.as<Real>(); t.gfat = p.tg.as<Real>(); t.Qbuf = p.tQ.as<Real>();
  t.S1 = p.tS1.as<Real>(); t.S2 = p.tS2.as<Real>(); t.sv = p.tsv.as<Real>(); t.xfat = p.tx.as<Real>();
  return t;
}

// one level of the fat blocks' cyclic reduction: blocks up to 48 columns are factored in registers (k_fat_elim_rows), wider
// ones through LDS (k_fat_elim_mfma, k_fat_elim_wide_mfma)
template <typename RowT> void launch_fat_elim(const FsArgs<Real, RowT> &a, const FatLevel &fl, hipStream_t st) {
  const int nbp = (a.NB + 7) & ~7;
  if (nbp <= 48) {
    switch (nbp) {
      case 8: k_fat_elim_rows<8, RowT><<<dim3(fl.nelim), dim3(256), 0, st>>>(a, fl); break;
      case 16: k_fat_elim_rows<16, RowT><<<dim3(fl.nelim), dim3(256), 0, st>>>(a, fl); break;
      case 24: k_fat_elim_rows<24, RowT><<<dim3(fl.nelim), dim3(256), 0, st>>>(a, fl); break;
      case 32: k_fat_elim_rows<32, RowT><<<dim3(fl.nelim), dim3(256), 0, st>>>(a, fl); break;
      case 40: k_fat_elim_rows<40, RowT><<<dim3(fl.nelim), dim3(256), 0, st>>>(a, fl); break;
      default: k_fat_elim_rows<48, RowT><<<dim3(fl.nelim), dim3(512), 0, st>>>(a, fl); break;
    }
    return;
  }
  if (a.NB > kFatLds) {   // the factor in LDS, [H | H | g] through it in panels of PW columns
    const int PW = fat_wide_panel((int)sizeof(Real), a.NB);
    k_fat_elim_wide_mfma<RowT><<<dim3(fl.nelim), dim3(1024), fat_elim_wide_lds(a.NB), st>>>(a, fl, PW);
    return;
  }
  k_fat_elim_mfma<RowT><<<dim3(fl.nelim), dim3(1024), fat_elim_mfma_lds(a.NB), st>>>(a, fl);
}

template <typename RowT> void launch_fat_back(const FsArgs<Real, RowT> &a, const FatLevel &fl, hipStream_t st) {
  const int nbp = (a.NB + 7) & ~7;
  if (nbp <= 48) {
    switch (nbp) {
      case 8: case 16: k_fat_back_rows<16, RowT><<<dim3(fl.nelim), dim3(64), 0, st>>>(a, fl); break;
      case 24: k_fat_back_rows<24, RowT><<<dim3(fl.nelim), dim3(64), 0, st>>>(a, fl); break;
      case 32: k_fat_back_rows<32, RowT><<<dim3(fl.nelim), dim3(64), 0, st>>>(a, fl); break;
      case 40: k_fat_back_rows<40, RowT><<<dim3(fl.nelim), dim3(64), 0, st>>>(a, fl); break;
      default: k_fat_back_rows<48, RowT><<<dim3(fl.nelim), dim3(64), 0, st>>>(a, fl); break;
    }
    return;
  }
  k_fat_back_w4<RowT><<<dim3(fl.nelim), dim3(256), fat_back_w4_lds(a.NB), st>>>(a, fl);
}

// The cyclic reduction over a list of level sets, and the back-substitution over it once the block(s) it stopped at are solved.  The
// chain's fat blocks (p.levels) and a split chain's top system (p.tlevels, with fs_top_args) both come through here.
template <typename RowT>
void fat_reduce(const FsArgs<Real, RowT> &a, const std::vector<FatSepPlan::LevelHost> &levels, const DevBuf &elim, const DevBuf &upd, hipStream_t st) {
  for (const FatSepPlan::LevelHost &lv : levels) {
    const FatLevel fl = fat_level(lv, elim, &upd);
    launch_fat_elim(a, fl, st);
    if (lv.nupd > 0) k_fat_update<Real, RowT><<<dim3(lv.nupd), dim3(256), 0, st>>>(a, fl);
  }
}
template <typename RowT>
void fat_substitute(const FsArgs<Real, RowT> &a, const std::vector<FatSepPlan::LevelHost> &levels, const DevBuf &elim, hipStream_t st) {
  for (int li = (int)levels.size() - 1; li >= 0; li--) launch_fat_back(a, fat_level(levels[li], elim), st);
}

// segment interiors of the segmented landmark elimination: planar fp64 chains take the cooperative row-layout kernel (four
// segments per wave), everything else the wave-per-segment kernel
template <int BB, typename T, typename TR> void fs_launch_factor(const FsArgs<T, TR> &a, int nseg, hipStream_t st) {
  if constexpr (BB == 6 && std::is_same<T, double>::value && std::is_same<TR, double>::value) {
    k_fs_factor_rows6<<<dim3((nseg + 3) / 4), dim3(64), 0, st>>>(a);
    return;
  }
  k_fs_factor<T, BB, TR><<<dim3(nseg), dim3(64), 0, st>>>(a);
}

// forward half: segment interiors -> fat blocks -> cyclic-reduction levels (down to one block, or to the two end blocks of a
// piece of a split chain)
// y_own: the sweep and the Schur complements in two launches through THIS Y buffer, whatever the plan's choice (marginals_fs.hip: the
// half-swept border Y = L^-1 G into the marginals' own buffer, zeroed by the caller -- a fused_sweep plan has none)
template <typename RowT> int fs_forward_rows(gpslam_hip_handle *h, double lambda, Real *y_own) {
  FatSepPlan &p = h->fs;
  FsArgs<Real, RowT> a = fs_args<RowT>(h, lambda);
  const bool fused_sweep = p.fused_sweep && !y_own;
  if (y_own) a.Y = y_own;
  hipStream_t st = h->stream;
  const int nseg = p.K - 1;
  // round 6: the segments' factorisation is a latency chain on one wave per SIMD (config 4: 1203 waves, 208 steps, 0.42 ms) and needs
  // nothing but the block records: the two kernels that only read the row tables -- the border's right-hand-side groups (k_fs_gev,
  // 42 us) and the landmarks' own terms (k_fs_lm_terms, 31 us) -- run on the second stream underneath it, joined in front of the sweep
  const bool lm_terms = a.fa_ptr != nullptr && h->L > 0;
  const bool side = h->aux_stream != nullptr && (p.ngroups > 0 || lm_terms) && h->N >= kForkMinStates;
  hipStream_t st2 = side ? h->aux_stream : st;
  if (side) {
    HIPCHK(hipEventRecord(h->ev_fork, st));
    HIPCHK(hipStreamWaitEvent(h->aux_stream, h->ev_fork, 0));
  }
  dispatch_b(h->b, [&](auto tag) {
    constexpr int BB = decltype(tag)::value;
    if (p.ngroups > 0) k_fs_gev<Real, BB, RowT><<<dim3(nblocks(p.ngroups * h->ld, 256)), dim3(256), 0, st2>>>(a);
    if (side && lm_terms) k_fs_lm_terms<Real, RowT><<<dim3(nblocks(h->L, 128)), dim3(128), 0, st2>>>(a);
    fs_launch_factor<BB>(a, nseg, st);
    if (side) {
      (void)hipEventRecord(h->ev_join, h->aux_stream);
      (void)hipStreamWaitEvent(st, h->ev_join, 0);
    }
    if (!fused_sweep) k_fs_sweep<Real, BB, RowT><<<dim3(nseg), dim3(((p.NC + 63) / 64) * 64), 0, st>>>(a);
  });
  if (fused_sweep) {   // sweep + Schur complement in one launch (planar chains, borders up to 112 columns): no Y buffer
    const size_t smem = fs_fused_smem(h->b, p.NCP);
    switch (p.NCP / 16) {
      case 2: k_fs_sweep_syrk<6, 2, RowT><<<dim3(nseg), dim3(256), smem, st>>>(a); break;
      case 3: k_fs_sweep_syrk<6, 3, RowT><<<dim3(nseg), dim3(256), smem, st>>>(a); break;
      case 4: k_fs_sweep_syrk<6, 4, RowT><<<dim3(nseg), dim3(256), smem, st>>>(a); break;
      case 5: k_fs_sweep_syrk<6, 5, RowT><<<dim3(nseg), dim3(256), smem, st>>>(a); break;
      case 6: k_fs_sweep_syrk<6, 6, RowT><<<dim3(nseg), dim3(256), smem, st>>>(a); break;
      default: k_fs_sweep_syrk<6, 7, RowT><<<dim3(nseg), dim3(256), smem, st>>>(a); break;
    }
  } else {   // accumulator tiles per wave and staged row width: the smallest instantiation that covers this border (config 4: 15 tiles, 80 columns)
    // two instantiations (accumulator tiles per wave, widest staged row = LDS row stride).  Measured at config 4 (NCP = 80, 15
    // tiles, 1e6 states): <7, 112> 6.0 ms per iteration, <12, 144> 6.2 ms, and a <4, 80> that compiles to a loop twice as slow
    // (8.1 ms: four accumulators per wave leave the matrix pipeline's latency exposed) and is not instantiated.
    const int ncm = p.NCP <= 112 ? 112 : (p.NCP <= 144 ? 144 : (p.NCP <= 176 ? 176 : 272));
    const size_t smem = fs_syrk_lds(ncm);
    if (ncm == 112) k_fs_syrk<7, 112, RowT><<<dim3(nseg), dim3(256), smem, st>>>(a);          // <= 28 tiles / 4 waves
    else if (ncm == 144) k_fs_syrk<12, 144, RowT><<<dim3(nseg), dim3(256), smem, st>>>(a);    // <= 45 tiles
    else if (ncm == 176) k_fs_syrk<17, 176, RowT><<<dim3(nseg), dim3(256), smem, st>>>(a);    // <= 66 tiles (NB up to 80)
    else k_fs_syrk<20, 272, RowT><<<dim3(nseg, 2), dim3(256), smem, st>>>(a);                  // <= 153 tiles over two workgroups (NB up to 128)
  }
  if (lm_terms && !side) k_fs_lm_terms<Real, RowT><<<dim3(nblocks(h->L, 128)), dim3(128), 0, st>>>(a);
  k_fs_fat_assemble<Real, RowT><<<dim3(p.K), dim3(256), 0, st>>>(a);
  fat_reduce(a, p.levels, p.d_elim, p.d_upd, st);
  HIPCHK(hipGetLastError());
  return 0;
}

// backward half, once xfat of the block(s) the forward half stopped at is known
template <typename RowT> int fs_backward(gpslam_hip_handle *h, double lambda) {
  FatSepPlan &p = h->fs;
  FsArgs<Real, RowT> a = fs_args<RowT>(h, lambda);
  hipStream_t st = h->stream;
  const int nseg = p.K - 1;
  fat_substitute(a, p.levels, p.d_elim, st);
  k_fs_scatter<Real, RowT><<<dim3(nblocks(std::max(p.K * h->b, h->L * h->ld), 256)), dim3(256), 0, st>>>(a);
  dispatch_b(h->b, [&](auto tag) {
    constexpr int BB = decltype(tag)::value;
    k_fs_rhs<Real, BB, RowT><<<dim3(nblocks(h->N, 128)), dim3(128), 0, st>>>(a);
    k_fs_solve1<Real, BB, RowT><<<dim3(nseg), dim3(64), 0, st>>>(a);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

// The dynamic-LDS attributes of one row type's kernels.  Process-wide per kernel: always the size of the LARGEST fat block and of the
// widest border an instantiation serves, whatever this handle's (a later handle with a narrower border must not lower what
// an earlier one needs)
template <typename RowT> int fs_set_lds_attributes(gpslam_hip_handle *h) {
  const std::pair<const void *, size_t> lds[] = {
      {reinterpret_cast<const void *>(&k_fat_elim_mfma<RowT>), fat_elim_mfma_lds(kFatLds)},
      {reinterpret_cast<const void *>(&k_fat_elim_wide_mfma<RowT>), fat_elim_wide_lds(kFatMax)},
      {reinterpret_cast<const void *>(&k_fat_top<Real, RowT>), fat_top_lds(kFatMax)},
      {reinterpret_cast<const void *>(&k_fat_back_w4<RowT>), fat_back_w4_lds(kFatMax)},
      {reinterpret_cast<const void *>(&k_fs_syrk<7, 112, RowT>), fs_syrk_lds(112)},
      {reinterpret_cast<const void *>(&k_fs_syrk<12, 144, RowT>), fs_syrk_lds(144)},
      {reinterpret_cast<const void *>(&k_fs_syrk<17, 176, RowT>), fs_syrk_lds(176)},
      {reinterpret_cast<const void *>(&k_fs_syrk<20, 272, RowT>), fs_syrk_lds(272)},
      {reinterpret_cast<const void *>(&k_fs_sweep_syrk<6, 2, RowT>), fs_fused_smem(6, 32)},
      {reinterpret_cast<const void *>(&k_fs_sweep_syrk<6, 3, RowT>), fs_fused_smem(6, 48)},
      {reinterpret_cast<const void *>(&k_fs_sweep_syrk<6, 4, RowT>), fs_fused_smem(6, 64)},
      {reinterpret_cast<const void *>(&k_fs_sweep_syrk<6, 5, RowT>), fs_fused_smem(6, 80)},
      {reinterpret_cast<const void *>(&k_fs_sweep_syrk<6, 6, RowT>), fs_fused_smem(6, 96)},
      {reinterpret_cast<const void *>(&k_fs_sweep_syrk<6, 7, RowT>), fs_fused_smem(6, 112)}};
  for (const auto &kl : lds) HIPCHK(hipFuncSetAttribute(kl.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kl.second));
  return 0;
}

template <typename T> void lmprior_err(gpslam_hip_handle *h, int nbl, T *partial, hipStream_t st) {
  k_fs_lmprior_err<T><<<dim3(nbl), dim3(256), 0, st>>>(h->lmk.as<double>(), h->lpri.d_idx.as<int>(), h->lpri.d_meas.as<double>(),
                                                        h->lpri.d_sig.as<double>(), h->lpri.count(), h->ld, partial);
}

}  // namespace

int fs_forward(gpslam_hip_handle *h, double lambda, double *y_own) {
  return dispatch_row(h, [&](auto row) -> int { return fs_forward_rows<typename decltype(row)::type>(h, lambda, y_own); });
}

int fs_solve(gpslam_hip_handle *h, double lambda) {
  FatSepPlan &p = h->fs;
  // a piece's cyclic reduction stops at its two end blocks: without the neighbours' records there is nothing to solve
  if (p.split) return fail(h, GPSLAM_E_INVALID, "piece of a split chain: use fs_phase1 / fs_phase2 (or the fs_lm_trial steps)");
  return dispatch_row(h, [&](auto row) -> int {
    typedef typename decltype(row)::type RowT;
    int rc;
    if ((rc = fs_forward_rows<RowT>(h, lambda, nullptr))) return rc;
    k_fat_top<Real, RowT><<<dim3(1), dim3(256), fat_top_lds(p.NB), h->stream>>>(fs_args<RowT>(h, lambda), p.top);
    return fs_backward<RowT>(h, lambda);
  });
}

// the piece's interface record (its two end blocks and the link between them, padded to the top block size) into the send buffer
int fs_pack_record(gpslam_hip_handle *h) {
  FatSepPlan &p = h->fs;
  return dispatch_row(h, [&](auto row) -> int {
    typedef typename decltype(row)::type RowT;
    k_fs_pack_record<Real, RowT><<<dim3(nblocks(p.nb_top * p.nb_top, 256)), dim3(256), 0, h->stream>>>(fs_args<RowT>(h, h->ph_lambda), p.end_link, p.nb_top,
                                                                                                        p.send.as<Real>());
    HIPCHK(hipGetLastError());
    return 0;
  });
}

int fs_split_solve(gpslam_hip_handle *h) {
  FatSepPlan &p = h->fs;
  hipStream_t s = h->stream;
  const int NT = p.nb_top, P = p.nranks;
  return dispatch_row(h, [&](auto row) -> int {
    typedef typename decltype(row)::type RowT;
    FsArgs<Real, RowT> t = fs_top_args<RowT>(h);
    k_fs_top_build<Real><<<dim3(P + 1), dim3(256), 0, s>>>(p.recv.as<Real>(), P, NT, t.Dfat, t.link, t.gfat);
    fat_reduce(t, p.tlevels, p.d_telim, p.d_tupd, s);
    k_fat_top<Real, RowT><<<dim3(1), dim3(256), fat_top_lds(NT), s>>>(t, p.ttop);
    fat_substitute(t, p.tlevels, p.d_telim, s);
    k_fs_top_take<Real, RowT><<<dim3(1), dim3(64), 0, s>>>(fs_args<RowT>(h, h->ph_lambda), t.xfat, p.rank, NT);
    return fs_backward<RowT>(h, h->ph_lambda);
  });
}

void fs_lmprior_err(gpslam_hip_handle *h, int nbl, double *partial, hipStream_t st) { lmprior_err(h, nbl, partial, st); }
void fs_lmprior_err(gpslam_hip_handle *h, int nbl, float *partial, hipStream_t st) { lmprior_err(h, nbl, partial, st); }

void fs_lm_update(gpslam_hip_handle *h, int slot, hipStream_t st) {
  const int nbl = std::min(nblocks(h->nl, 256), 1024);
  k_fs_lm_update<Real><<<dim3(nbl), dim3(256), 0, st>>>(h->lmk.as<double>(), h->lm_dL.as<Real>(), h->nl, h->flag.as<int>(), h->fs.partial.as<Real>());
  k_fs_max_into<Real><<<dim3(1), dim3(64), 0, st>>>(h->fs.partial.as<Real>(), nbl, h->scal.as<double>() + slot);
}

void fs_mask_mul(gpslam_hip_handle *h, const double *dL, hipStream_t st) {
  k_fs_mask_mul<Real><<<dim3(nblocks(h->nl, 256)), dim3(256), 0, st>>>(dL, h->fs.d_lm_own.as<int>(), h->ld, h->nl, h->fs.lm_tmp.as<Real>());
}

// ---- a chain split into pieces: what the caller asks and sets before the phase calls (api_iterate.inc).  Nothing here depends on
// the rows' type.  compile() has planned this piece with its end blocks kept (FatSepPlan::split); set_top sizes the interface
// record once the caller knows the widest fat block of any piece.
int gpslam_hip_fs_split_info(gpslam_hip_handle *h, int32_t out4[4]) {
  int rc = need_compiled(h);
  if (rc) return rc;
  if (!out4 || !split_piece(h)) return GPSLAM_E_INVALID;
  out4[0] = h->fs.NB; out4[1] = h->fs.K; out4[2] = h->fs.C; out4[3] = h->fs.nb_top;
  return 0;
}
int gpslam_hip_fs_set_top(gpslam_hip_handle *h, int32_t nb_top) {
  int rc = need_local(h);
  if (rc) return rc;
  FatSepPlan &p = h->fs;
  if (!split_piece(h)) return fail(h, GPSLAM_E_INVALID, "fs_set_top: not a piece of a split chain (gpslam_hip_fs_set_split before compile)");
  if (nb_top < p.NB || nb_top > kFatMax) return fail(h, GPSLAM_E_INVALID, "fs_set_top: the top block size must lie between this piece's fat block size and 128");
  const int P = p.nranks, NT = nb_top;
  const size_t NT2 = (size_t)NT * NT, RS = 3 * NT2 + 2 * NT;
  p.nb_top = NT;
  std::vector<int> elim, upd;
  int nlinks = 0, endl = 0;
  FatSepPlan::build_levels(P + 1, false, elim, upd, p.tlevels, p.ttop, nlinks, endl);
  if (elim.empty()) elim.assign(6, 0);
  if (upd.empty()) upd.assign(3, 0);
  HIPCHK(upload_vec(h->stream, p.d_telim, elim));
  HIPCHK(upload_vec(h->stream, p.d_tupd, upd));
  HIPCHK(p.send.reserve(RS * sizeof(Real)));
  HIPCHK(p.recv.reserve((size_t)P * RS * sizeof(Real)));
  HIPCHK(p.tD.reserve((size_t)(P + 1) * NT2 * sizeof(Real)));
  HIPCHK(p.tlink.reserve((size_t)std::max(nlinks, P) * NT2 * sizeof(Real)));
  HIPCHK(p.tg.reserve((size_t)(P + 1) * NT * sizeof(Real)));
  HIPCHK(p.tQ.reserve((size_t)(P + 1) * NT2 * sizeof(Real)));
  HIPCHK(p.tS1.reserve((size_t)(P + 1) * NT2 * sizeof(Real)));
  HIPCHK(p.tS2.reserve((size_t)(P + 1) * NT2 * sizeof(Real)));
  HIPCHK(p.tsv.reserve((size_t)(P + 1) * 2 * NT * sizeof(Real)));
  HIPCHK(p.tx.reserve((size_t)(P + 1) * NT * sizeof(Real)));
  // (the dynamic-LDS attributes of the elimination kernels and of k_fat_top were set to the largest fat block's size by compile(): fs_build)
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// compile(): segment plan, level sets of the cyclic reduction, buffers.  per_lm: rows touching each landmark (row, left
// state), sorted by state; touch_hi: last state touched.
int fs_build(gpslam_hip_handle *h, const std::vector<int> &touch_lo, const std::vector<int> &touch_hi) {
  FatSepPlan &p = h->fs;
  const int N = h->N, b = h->b, ld = h->ld, L = h->L;
  std::vector<int> fat_of, slot_of, counts;
  if (!p.choose(N, b, ld, L, touch_lo, touch_hi, h->cfg.segment_length, fat_of, slot_of, counts)) return fail(h, GPSLAM_E_UNSUPPORTED, p.err.c_str());
  const int K = p.K, NB = p.NB;
  std::vector<int> segid(N, 0);
  for (int k = 0; k + 1 < K; k++)
    for (int s2 = p.cuts[k] + 1; s2 < p.cuts[k + 1]; s2++) segid[s2] = k;
  for (int k = 0; k < K; k++) segid[p.cuts[k]] = -1 - k;
  std::vector<int> fat_ptr(K + 1, 0), fat_lm(L, 0);
  for (int k = 0; k < K; k++) fat_ptr[k + 1] = fat_ptr[k] + counts[k];
  for (int l = 0; l < L; l++) fat_lm[fat_ptr[fat_of[l]] + slot_of[l]] = l;
  std::vector<int> pri_ptr(L + 1, 0), pri_ids(h->lpri.idx.size());
  for (int32_t i : h->lpri.idx) pri_ptr[i + 1]++;
  for (int l = 0; l < L; l++) pri_ptr[l + 1] += pri_ptr[l];
  { std::vector<int> cur(pri_ptr.begin(), pri_ptr.end() - 1);
    for (size_t k = 0; k < h->lpri.idx.size(); k++) pri_ids[cur[h->lpri.idx[k]]++] = (int)k; }
  // level sets of the block cyclic reduction (a piece of a split chain keeps its two end blocks)
  std::vector<int> elim, upd;
  FatSepPlan::build_levels(K, p.split, elim, upd, p.levels, p.top, p.nlinks, p.end_link);
  hipStream_t st = h->stream;
  HIPCHK(upload_vec(st, p.d_cuts, p.cuts));
  HIPCHK(upload_vec(st, p.d_segid, segid));
  HIPCHK(upload_vec(st, p.d_fat_lm_ptr, fat_ptr));
  HIPCHK(upload_vec(st, p.d_fat_lm, fat_lm));
  HIPCHK(upload_vec(st, p.d_lm_fat, fat_of));
  HIPCHK(upload_vec(st, p.d_lm_slot, slot_of));
  p.h_lm_fat = fat_of; p.h_lm_slot = slot_of;
  HIPCHK(upload_vec(st, p.d_lmpri_ptr, pri_ptr));
  HIPCHK(upload_vec(st, p.d_lmpri, pri_ids));
  std::vector<int> lg_ptr(L + 1, 0), lg_state;
  {   // right-hand-side groups of the landmark border columns: row rho puts its left half on its own state and its right
      // half on the next one; per landmark the events are ordered by state (stable: the rows of state s - 1 before those of
      // state s, the order the sweep used to add them in) and events on one state form a group
    std::vector<int> lg_mptr(1, 0), lg_m;
    std::vector<std::pair<int, int>> ev;
    for (int l = 0; l < L; l++) {
      ev.clear();
      for (int t = p.h_lmptr[l]; t < p.h_lmptr[l + 1]; t++) {
        ev.push_back({p.h_lmstate[t], p.h_lmrow[t] * 2});
        if (p.h_lmstate[t] + 1 < N) ev.push_back({p.h_lmstate[t] + 1, p.h_lmrow[t] * 2 + 1});
      }
      std::stable_sort(ev.begin(), ev.end(), [](const std::pair<int, int> &x, const std::pair<int, int> &y) { return x.first < y.first; });
      for (size_t k = 0; k < ev.size(); k++) {
        if (k == 0 || ev[k].first != ev[k - 1].first) {
          if (k) lg_mptr.push_back((int)lg_m.size());
          lg_state.push_back(ev[k].first);
        }
        lg_m.push_back(ev[k].second);
      }
      if (!ev.empty()) lg_mptr.push_back((int)lg_m.size());
      lg_ptr[l + 1] = (int)lg_state.size();
    }
    p.ngroups = (int)lg_state.size();
    if (lg_state.empty()) lg_state.push_back(0);
    if (lg_m.empty()) lg_m.push_back(0);
    if (lg_mptr.size() < 2) lg_mptr.push_back(0);
    HIPCHK(upload_vec(st, p.d_lg_ptr, lg_ptr));
    HIPCHK(upload_vec(st, p.d_lg_state, lg_state));
    HIPCHK(upload_vec(st, p.d_lg_mptr, lg_mptr));
    HIPCHK(upload_vec(st, p.d_lg_m, lg_m));
    HIPCHK(p.Gev.reserve((size_t)std::max(p.ngroups, 1) * ld * b * sizeof(Real)));
    HIPCHK(hipMemsetAsync(p.Gev.p, 0, (size_t)std::max(p.ngroups, 1) * ld * b * sizeof(Real), st));
  }
  {   // rows of each landmark that touch its own / the next / the previous cut state, by position of the landmark in fat_lm
    if (L == 0) {   // freed now: without landmarks there are no such rows, and an earlier compile() may have left its tables
      for (DevBuf *bf : {&p.d_fa_ptr, &p.d_fa_it, &p.d_fb_ptr, &p.d_fb_it, &p.d_fc_ptr, &p.d_fc_it}) bf->release();
    } else {
      std::vector<int> ptr[3], it[3];
      for (int w = 0; w < 3; w++) ptr[w].assign(L + 1, 0);
      for (int pos = 0; pos < L; pos++) {
        const int l = fat_lm[pos], kf = fat_of[l];
        const int c[3] = {p.cuts[kf], kf + 1 < K ? p.cuts[kf + 1] : -10, kf > 0 ? p.cuts[kf - 1] : -10};
        for (int t = p.h_lmptr[l]; t < p.h_lmptr[l + 1]; t++) {
          const int ls = p.h_lmstate[t], rho = p.h_lmrow[t];
          for (int w = 0; w < 3; w++) {
            if (c[w] < 0) continue;
            if (ls == c[w]) it[w].push_back(rho * 2);
            else if (ls == c[w] - 1) it[w].push_back(rho * 2 + 1);
          }
        }
        for (int w = 0; w < 3; w++) ptr[w][pos + 1] = (int)it[w].size();
      }
      for (int w = 0; w < 3; w++) if (it[w].empty()) it[w].push_back(0);
      HIPCHK(upload_vec(st, p.d_fa_ptr, ptr[0])); HIPCHK(upload_vec(st, p.d_fa_it, it[0]));
      HIPCHK(upload_vec(st, p.d_fb_ptr, ptr[1])); HIPCHK(upload_vec(st, p.d_fb_it, it[1]));
      HIPCHK(upload_vec(st, p.d_fc_ptr, ptr[2])); HIPCHK(upload_vec(st, p.d_fc_it, it[2]));
      HIPCHK(p.lmMM.reserve((size_t)L * ld * ld * sizeof(Real)));
    }
  }
  if (p.split) {
    std::vector<int> own(std::max(L, 1), 1);
    if (p.rank < p.nranks - 1) for (int l : p.last_lm) own[l] = 0;      // the piece on the right reports / counts them
    HIPCHK(upload_vec(st, p.d_lm_own, own));
    HIPCHK(p.lm_tmp.reserve((size_t)std::max(h->nl, 1) * sizeof(Real)));
  }
  HIPCHK(upload_vec(st, p.d_elim, elim));
  HIPCHK(upload_vec(st, p.d_upd, upd));
  const size_t NB2 = (size_t)NB * NB;
  HIPCHK(p.fac.reserve((size_t)N * 2 * b * b * sizeof(Real)));
  {   // k_fs_sweep_syrk: planar chains (block size 6), borders up to 112 columns.  GPSLAM_PLAN_FS_TWO_LAUNCHES: the two launches
      // through the Y buffer (N x B x NCP doubles) that wider borders and other block sizes take
    const bool off = plan_bit(h, GPSLAM_PLAN_FS_TWO_LAUNCHES);
    p.fused_sweep = !off && b == 6 && p.NCP <= 112 && p.NC <= 128 && p.NCP >= 32;
  }
  if (p.fused_sweep) {
    // entries per chunk of 24 / b states: every group of a landmark that lands on an interior state of a segment next to the
    // landmark's cut, once per landmark component
    const int SPC = 24 / b;
    std::vector<int> sc_base(K, 0);
    for (int k = 0; k + 1 < K; k++) {
      const int nint = p.cuts[k + 1] - p.cuts[k] - 1;
      sc_base[k + 1] = sc_base[k] + (nint > 0 ? (nint + SPC - 1) / SPC : 0);
    }
    const int nch = sc_base[K - 1];
    std::vector<int> sc_ptr(nch + 2, 0);
    const std::vector<int> &g_state = lg_state, &g_ptr = lg_ptr;
    auto chunk_of = [&](int l, int sidx, int &col0, int &jj) -> int {     // -1: the group is not a border right-hand side
      const int sg = segid[sidx];
      if (sg < 0) return -1;
      const int kf = fat_of[l];
      if (kf != sg && kf != sg + 1) return -2;
      col0 = (kf == sg ? 0 : NB) + b + slot_of[l] * ld;
      jj = sidx - (p.cuts[sg] + 1);
      return sc_base[sg] + jj / SPC;
    };
    for (int pass = 0; pass < 2; pass++) {
      std::vector<int> cur(sc_ptr.begin(), sc_ptr.end());
      std::vector<int> se_pk, se_src;
      if (pass == 1) { se_pk.assign((size_t)sc_ptr[nch] + 64, 0); se_src.assign((size_t)sc_ptr[nch] + 64, 0); }
      for (int l = 0; l < L; l++)
        for (int gi = g_ptr[l]; gi < g_ptr[l + 1]; gi++) {
          int col0 = 0, jj = 0;
          const int ci = chunk_of(l, g_state[gi], col0, jj);
          if (ci == -2) return fail(h, GPSLAM_E_UNSUPPORTED, "segmented elimination: a landmark's factor lies outside the two segments next to its cut");
          if (ci < 0) continue;
          for (int q = 0; q < ld; q++) {
            if (pass == 0) sc_ptr[ci + 1]++;
            else { se_pk[cur[ci]] = (jj << 8) | (col0 + q); se_src[cur[ci]] = gi * ld + q; cur[ci]++; }
          }
        }
      if (pass == 0) { for (int ci = 0; ci < nch; ci++) sc_ptr[ci + 1] += sc_ptr[ci]; sc_ptr[nch + 1] = sc_ptr[nch]; }
      else {
        HIPCHK(upload_vec(st, p.d_se_pk, se_pk));
        HIPCHK(upload_vec(st, p.d_se_src, se_src));
      }
    }
    HIPCHK(upload_vec(st, p.d_sc_base, sc_base));
    HIPCHK(upload_vec(st, p.d_sc_ptr, sc_ptr));
    p.Y.release();   // freed now: the fused sweep never reads Y, and it is the plan's largest buffer
  } else {
    HIPCHK(p.Y.reserve((size_t)N * b * p.NCP * sizeof(Real)));
    HIPCHK(hipMemsetAsync(p.Y.p, 0, (size_t)N * b * p.NCP * sizeof(Real), st));   // padding columns stay zero for good
  }
  HIPCHK(p.Aseg.reserve((size_t)(K - 1) * p.NCP * p.NCP * sizeof(Real)));
  HIPCHK(p.Dfat.reserve((size_t)K * NB2 * sizeof(Real)));
  HIPCHK(p.link.reserve((size_t)p.nlinks * NB2 * sizeof(Real)));
  HIPCHK(p.gfat.reserve((size_t)K * NB * sizeof(Real)));
  HIPCHK(p.Qbuf.reserve((size_t)K * NB2 * sizeof(Real)));
  HIPCHK(p.S1.reserve((size_t)K * NB2 * sizeof(Real)));
  HIPCHK(p.S2.reserve((size_t)K * NB2 * sizeof(Real)));
  HIPCHK(p.sv.reserve((size_t)K * 2 * NB * sizeof(Real)));
  HIPCHK(p.xfat.reserve((size_t)K * NB * sizeof(Real)));
  HIPCHK(p.rhs.reserve((size_t)N * b * sizeof(Real)));
  HIPCHK(p.partial.reserve(1024 * sizeof(Real)));
  HIPCHK(h->lm_gL.reserve((size_t)std::max(h->nl, 1) * sizeof(Real)));
  HIPCHK(h->lm_dL.reserve((size_t)std::max(h->nl, 1) * sizeof(Real)));
  // the dynamic-LDS attributes of this handle's row type
  if (int rc = dispatch_row(h, [&](auto row) -> int { return fs_set_lds_attributes<typename decltype(row)::type>(h); })) return rc;
  p.active = true;
  return 0;
}
