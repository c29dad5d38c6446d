// fatsep_plan.hpp -- the host side of the segmented landmark elimination (fatsep.hpp has the kernels, fatsep.hip launches them): the
// plan compile() makes of a graph (FatSepPlan: cuts, landmarks per cut, level sets of the cyclic reduction, buffers), the argument
// of one reduction level (FatLevel) and the sizes the host plans with.  No kernel and no device function: every unit reads this
// through api_common.hpp, and only fatsep.hip reads fatsep.hpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "devbuf.hpp"

namespace gps {

constexpr int kFatMax = 128;  // largest fat block (cut state + landmark columns): what one workgroup's LDS holds of ONE NB x NB operand
                              // (k_fat_elim_wide_mfma, k_fat_top, k_fat_back_w4: 132 KB of 160).  Config 4's graph needs 28-36, twice its
                              // landmark density 62, three times 96-100.
// columns of [H | H | g] per pass of k_fat_elim_wide_mfma: what is left of 160 KB beside the block (and the 4 x 4 factors in Ld)
inline int fat_wide_panel(int elem_bytes, int NB) {
  const long avail = 160L * 1024 - (long)(kFatMax / 4) * 10 * elem_bytes - (long)NB * (NB + 1) * elem_bytes - 512;
  long pw = avail / ((long)NB * elem_bytes);
  if (pw > 2 * NB + 1) pw = 2 * NB + 1;
  return (int)(pw < 4 ? 4 : pw);
}
constexpr int kFatLds = 80;   // round 3: 64 -> 80, what the LDS holds of all three NB x NB operands of k_fat_elim_mfma (155 KB of 160).
                              // Round 5: wider blocks keep the factor in LDS and stream [H | H | g] through it in column panels
                              // (k_fat_elim_wide_mfma).

// ---- block cyclic reduction over the fat blocks.  One level: eliminate every other active block m (left neighbour l,
// right neighbour r or -1):  D_m = L L^T,  P = L^-1 H[m, l],  Q = L^-1 H[m, r],  z = L^-1 g_m;
// S1 = P^T P -> D_l,  S2 = Q^T Q -> D_r,  new link H[r, l] = -Q^T P,  P^T z -> g_l,  Q^T z -> g_r.
struct FatLevel {
  const int *elim;     // 6 ints per eliminated block: m, l, r, link(l -> m), link(m -> r), new link(l -> r)
  int nelim;
  const int *upd;      // 3 ints per survivor: a, eliminated block on its left (or -1), on its right (or -1)
  int nupd;
};

struct FatSepPlan {
  bool active = false;
  int N = 0, B = 0, ld = 0, L = 0, K = 0, NB = 0, NC = 0, NCP = 0, C = 0, nlinks = 0, top = 0;
  std::vector<int> cuts;
  struct LevelHost { int elim_off, nelim, upd_off, nupd; };
  std::vector<LevelHost> levels;
  DevBuf d_cuts, d_segid, d_fat_lm_ptr, d_fat_lm, d_lm_fat, d_lm_slot, d_lmpri_ptr, d_lmpri, d_elim, d_upd;
  DevBuf fac, Y, Aseg, Dfat, link, gfat, Qbuf, S1, S2, sv, xfat, gL, rhs, partial;
  std::string err;
  // a chain split across GPUs (gpslam_hip_fs_set_split): this handle holds piece `rank` of `nranks`; its first / last fat
  // block is shared with the neighbour piece and holds exactly the landmarks first_lm / last_lm, in that order
  bool split = false;
  int rank = 0, nranks = 1, nb_top = 0, end_link = 0, ttop = 0;
  std::vector<int> first_lm, last_lm;
  std::vector<LevelHost> tlevels;
  DevBuf send, recv, tD, tlink, tg, tQ, tS1, tS2, tsv, tx, d_telim, d_tupd, d_lm_own, lm_tmp;
  // right-hand-side groups of the landmark border columns (FsArgs::lg_*)
  DevBuf d_lg_ptr, d_lg_state, d_lg_mptr, d_lg_m, Gev;
  DevBuf d_sc_base, d_sc_ptr, d_se_pk, d_se_src;    // the same as entries per chunk (k_fs_sweep_syrk)
  DevBuf d_fa_ptr, d_fa_it, d_fb_ptr, d_fb_it, d_fc_ptr, d_fc_it;   // rows of each landmark that touch a cut state (k_fs_fat_assemble)
  DevBuf lmMM;
  bool fused_sweep = false;                         // k_fs_sweep_syrk serves this plan (else k_fs_sweep + k_fs_syrk through Y)
  int ngroups = 0;
  std::vector<int> h_lmrow, h_lmstate, h_lmptr;     // compile(): rows per landmark, sorted by left state
  std::vector<int> h_lm_fat, h_lm_slot;             // host copies of d_lm_fat / d_lm_slot (the marginals' landmark getters)

  // Level sets of the block cyclic reduction over K blocks in chain order: every level eliminates every other active block.
  // keep_last: the last block is never eliminated (a piece of a split chain stops at its two end blocks; end_link then is
  // the link between them).  elim: 6 ints per eliminated block, upd: 3 per survivor with an eliminated neighbour (FatLevel).
  static void build_levels(int K, bool keep_last, std::vector<int> &elim, std::vector<int> &upd, std::vector<LevelHost> &levels,
                           int &top, int &nlinks, int &end_link) {
    elim.clear(); upd.clear(); levels.clear();
    std::vector<int> active(K), linkidx(K > 0 ? K - 1 : 0);
    for (int k = 0; k < K; k++) active[k] = k;
    for (int k = 0; k + 1 < K; k++) linkidx[k] = k;
    int next_link = K - 1;
    while ((int)active.size() > (keep_last ? 2 : 1)) {
      LevelHost lv;
      lv.elim_off = (int)elim.size() / 6; lv.upd_off = (int)upd.size() / 3;
      const int n = (int)active.size();
      auto eliminated = [&](int q) { return q >= 0 && q < n && (q & 1) && !(keep_last && q == n - 1); };
      std::vector<int> nact, nlink;
      for (int i = 0; i < n; i++) {
        if (eliminated(i)) continue;
        nact.push_back(active[i]);
        if (!eliminated(i - 1) && !eliminated(i + 1)) continue;
        upd.push_back(active[i]);
        upd.push_back(eliminated(i - 1) ? active[i - 1] : -1);
        upd.push_back(eliminated(i + 1) ? active[i + 1] : -1);
      }
      for (int q = 1; q < n; q += 2) {
        if (!eliminated(q)) { nlink.push_back(linkidx[q - 1]); continue; }   // the kept last block: its link stays
        const int r = (q + 1 < n) ? active[q + 1] : -1;
        const int lk_new = (r >= 0) ? next_link++ : -1;
        elim.push_back(active[q]); elim.push_back(active[q - 1]); elim.push_back(r);
        elim.push_back(linkidx[q - 1]); elim.push_back(r >= 0 ? linkidx[q] : -1); elim.push_back(lk_new);
        if (r >= 0) nlink.push_back(lk_new);
      }
      lv.nelim = (int)elim.size() / 6 - lv.elim_off; lv.nupd = (int)upd.size() / 3 - lv.upd_off;
      levels.push_back(lv);
      active.swap(nact);
      linkidx.swap(nlink);
    }
    top = active[0];
    nlinks = std::max(next_link, 1);
    end_link = linkidx.empty() ? 0 : linkidx[0];
  }

  // even: segments of (nearly) equal length <= C instead of a short last one -- the pieces of a split chain, whose LAST
  // segment has to hold the whole window of every landmark shared with the neighbour
  static std::vector<int> make_cuts(int N, int C, bool even = false) {
    std::vector<int> c;
    if (even) {
      const int nseg = std::max(1, (N - 1 + C - 1) / C);
      for (int i = 0; i <= nseg; i++) c.push_back((int)(((long long)i * (N - 1)) / nseg));
      return c;
    }
    for (int s = 0; s < N - 1; s += C) c.push_back(s);
    if (c.empty() || c.back() != N - 1) c.push_back(N - 1);
    if (c.size() >= 3 && c[c.size() - 1] - c[c.size() - 2] < 2) c.erase(c.end() - 2);
    return c;
  }

  // touch_lo / touch_hi: first / last state touched by the factors of each landmark (-1: none).
  // Returns false (err set) when no segment length fits.
  bool choose(int N_, int B_, int ld_, int L_, const std::vector<int> &touch_lo, const std::vector<int> &touch_hi, int c_forced,
              std::vector<int> &fat_of, std::vector<int> &slot_of, std::vector<int> &counts) {
    N = N_; B = B_; ld = ld_; L = L_;
    if (N < 2) { err = "the segmented landmark elimination needs at least two states"; return false; }
    // one segmentation: cuts every Ctry states, every landmark on one admissible cut, balanced.  Returns whether every landmark
    // found a cut; nb_out = the fat block size it needs (B + ld * the fullest cut's landmarks)
    auto attempt = [&](int Ctry, int &nb_out) -> bool {
      cuts = make_cuts(N, Ctry, split);
      K = (int)cuts.size();
      counts.assign(K, 0);
      fat_of.assign(L, 0);
      slot_of.assign(L, 0);
      bool ok = true;
      // split chains: the shared end blocks hold exactly the listed landmarks, in the listed order (both neighbours build the
      // same block); every other landmark keeps away from them
      std::vector<int> forced(L, -1);
      const bool lsh = split && rank > 0, rsh = split && rank < nranks - 1;
      if (split) {
        for (int l : first_lm) {
          if (touch_lo[l] >= 0 && K >= 2 && touch_hi[l] > cuts[1]) { ok = false; break; }
          forced[l] = 0; fat_of[l] = 0; slot_of[l] = counts[0]++;
        }
        for (int l : last_lm) {
          if (!ok) break;
          if (touch_lo[l] >= 0 && K >= 2 && touch_lo[l] < cuts[K - 2]) { ok = false; break; }
          forced[l] = K - 1; fat_of[l] = K - 1; slot_of[l] = counts[K - 1]++;
        }
      }
      // The fat block size is set by the FULLEST cut (NB = B + ld * max count; the border of every segment, the Y buffer and
      // the cubic cost of the fat chain all scale with it), so the landmarks are balanced: those with a single admissible
      // cut first, then the others to the emptier of their cuts, then single moves off the fullest cuts while that lowers
      // the maximum (round 3: 17 -> 14 landmarks per cut on the config-4 graph, NB 40 -> 36).
      std::vector<int> lo_of(L, 0), hi_of(L, -1);
      for (int l = 0; l < L && ok; l++) {
        if (forced[l] >= 0) continue;
        int lo, hi;
        if (touch_lo[l] < 0) { lo = hi = std::min(std::max(l % K, lsh ? 1 : 0), rsh ? K - 2 : K - 1); }
        else {
          const int k_lo = (int)(std::upper_bound(cuts.begin(), cuts.end(), touch_lo[l]) - cuts.begin()) - 1;
          const int k_hi = (int)(std::lower_bound(cuts.begin(), cuts.end(), touch_hi[l]) - cuts.begin());
          if (k_hi - k_lo > 2) { ok = false; break; }
          lo = std::max(k_hi - 1, 0);
          hi = std::min(k_lo + 1, K - 1);
        }
        if (lsh && lo == 0) lo = 1;
        if (rsh && hi == K - 1) hi = K - 2;
        if (lo > hi) { ok = false; break; }
        lo_of[l] = lo; hi_of[l] = hi;
      }
      if (ok) {
        for (int pass = 0; pass < 2; pass++)          // pass 0: no choice; pass 1: the emptier admissible cut
          for (int l = 0; l < L; l++) {
            if (forced[l] >= 0 || (pass == 0) != (lo_of[l] == hi_of[l])) continue;
            int best = lo_of[l];
            for (int k = lo_of[l] + 1; k <= hi_of[l]; k++) if (counts[k] < counts[best]) best = k;
            fat_of[l] = best;
            counts[best]++;
          }
        std::vector<std::vector<int>> members(K);
        for (int l = 0; l < L; l++) if (forced[l] < 0) members[fat_of[l]].push_back(l);
        for (int round = 0; round < 64; round++) {    // move a landmark off a fullest cut to a cut at least two emptier
          int mxc = 0;
          for (int k = 0; k < K; k++) mxc = std::max(mxc, counts[k]);
          bool moved = false;
          for (int k = 0; k < K; k++) {
            if (counts[k] != mxc) continue;
            for (size_t q = 0; q < members[k].size(); q++) {
              const int l = members[k][q];
              int to = -1;
              for (int k2 = lo_of[l]; k2 <= hi_of[l]; k2++) if (k2 != k && counts[k2] + 1 < counts[k] && (to < 0 || counts[k2] < counts[to])) to = k2;
              if (to < 0) continue;
              members[k].erase(members[k].begin() + (long)q);
              members[to].push_back(l);
              fat_of[l] = to; counts[k]--; counts[to]++;
              moved = true;
              break;
            }
          }
          if (!moved) break;
        }
        // slots: forced landmarks keep theirs (the shared end blocks' order is the caller's); the rest in landmark order
        std::vector<int> next(K, 0);
        for (int k = 0; k < K; k++) next[k] = 0;
        for (int l = 0; l < L; l++) if (forced[l] >= 0) next[forced[l]]++;
        for (int l = 0; l < L; l++) if (forced[l] < 0) slot_of[l] = next[fat_of[l]]++;
      }
      int mx = 0;
      for (int k = 0; k < K; k++) mx = std::max(mx, counts[k]);
      nb_out = B + ld * mx;
      return ok;
    };
    const char *too_many = "too many landmarks per cut for the fat separators (2d + landmark_dim * landmarks must be <= 128)";
    auto no_fit = [&]() {
      return split ? "no segmentation of this piece keeps its private landmarks off the shared end blocks and the shared ones inside the "
                     "end segments: the piece is too short for the landmarks' windows of visibility (use fewer, longer pieces)"
                   : "a landmark is seen from more than two segments of the chain: no local-visibility segmentation exists";
    };
    // What a segmentation costs per state: the Schur complement of a segment is (NCP / 16)(NCP / 16 + 1) / 2 MFMA tiles per four
    // rows, the border sweep NC columns (measured on the config-4 graph: 0.064 ms per tile and 0.025 ms per column and 1e6
    // states) -- both set by the FULLEST cut, so a shorter segment with one landmark less on it can drop a whole tile row.
    auto score = [&](int nb) {
      const int nbr = std::min((nb + 3) & ~3, kFatMax), nc = 2 * nbr + 1, t = ((nc + 15) & ~15) / 16;
      return 0.064 * (t * (t + 1) / 2) + 0.025 * nc;
    };
    int nb = 0;
    if (c_forced > 0) {
      const bool ok = attempt(c_forced, nb);
      if (!ok || nb > kFatMax) { err = ok ? too_many : no_fit(); return false; }
      C = c_forced;
    } else {
      // doubling finds the first segment length that fits; the lengths between it and half of it (in sixteenths of it, at least 16
      // states) are then tried as well -- round 4: the config-4 graph fits at 256 (NB 36, 15 tiles) and at 208 (NB 28, 10 tiles:
      // the solve phase 3.32 -> 2.58 ms).  Among equal costs the longest segments win (fewer fat blocks).
      int Chi = 0;
      for (int Ctry = 32;; Ctry *= 2) {
        const bool ok = attempt(Ctry, nb);
        if (ok && nb <= kFatMax) { Chi = Ctry; break; }
        if (K <= 2) { err = ok ? too_many : no_fit(); return false; }
        if (ok && nb > kFatMax) { err = too_many; return false; }   // longer segments only add landmarks per cut
      }
      int best = Chi;
      double best_score = score(nb);
      const int step = std::max(16, Chi / 16);
      for (int Ctry = Chi - step; Ctry > Chi / 2; Ctry -= step) {
        const bool ok = attempt(Ctry, nb);
        if (!ok || nb > kFatMax) continue;
        if (score(nb) < best_score - 1e-12) { best = Ctry; best_score = score(nb); }
      }
      (void)attempt(best, nb);
      C = best;
    }
    NB = (nb + 3) & ~3;
    if (NB > kFatMax) NB = kFatMax;
    NC = 2 * NB + 1;
    NCP = (NC + 15) & ~15;
    return true;
  }
};

// one level of a plan's level sets as the kernels take it: the eliminated blocks out of `elim`, and the survivors to update out of
// `upd` (the forward reduction) or none (the back-substitution, the marginals' reverse walk)
inline FatLevel fat_level(const FatSepPlan::LevelHost &lv, const DevBuf &elim, const DevBuf *upd = nullptr) {
  FatLevel fl;
  fl.elim = elim.as<int>() + (size_t)6 * lv.elim_off; fl.nelim = lv.nelim;
  fl.upd = upd ? upd->as<int>() + (size_t)3 * lv.upd_off : nullptr; fl.nupd = upd ? lv.nupd : 0;
  return fl;
}

}  // namespace gps
