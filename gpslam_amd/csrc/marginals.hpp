// marginals.hpp -- the one home of gpslam_hip_marginals' state on the handle (h->mg) and of every layout its four translation units
// share (marginals.hip, marginals_clo.hip, marginals_fs.hip, marginals_pairs.hip).  Included by api_common.hpp in front of the handle;
// the device helpers the kernels share are in marginals_dev.hpp.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>

#include "devbuf.hpp"

struct gpslam_hip_handle;

namespace gps {

constexpr int kMgChunk = 16;        // states per chunk at every level of the selected inversion (the first one is the chunk's separator)
constexpr int kMgMaxLevels = 9;     // 16^8 > 2^31 states: an int N never needs more

// The levels of the selected inversion: n[0] = N, n[l + 1] = ceil(n[l] / kMgChunk), down to the one block of level `top`.  Level 0
// lives in the records and in Marginals::fac / S / Sn; every level above it has a slab of 8 B^2 doubles per block in Marginals::up, in
// the order D, O, add, fac (3: [P^-1 | U | V]), Sd, Sn -- the accessors give a part's offset into `up`, in doubles (l >= 1)
struct MgLevels {
  int n[kMgMaxLevels], top = 0;
  size_t off[kMgMaxLevels + 1], BB = 0;
  MgLevels(int N, int B) : BB((size_t)B * B) {
    n[0] = N;
    while (n[top] > 1) { n[top + 1] = (n[top] + kMgChunk - 1) / kMgChunk; top++; }
    off[0] = off[1] = 0;
    for (int l = 1; l <= top; l++) off[l + 1] = off[l] + 8 * BB * n[l];
  }
  size_t total() const { return off[top + 1]; }
  size_t D(int l) const { return off[l]; }
  size_t O(int l) const { return off[l] + BB * n[l]; }
  size_t add(int l) const { return off[l] + 2 * BB * n[l]; }
  size_t fac(int l) const { return off[l] + 3 * BB * n[l]; }
  size_t Sd(int l) const { return off[l] + 6 * BB * n[l]; }
  size_t Sn(int l) const { return off[l] + 7 * BB * n[l]; }
};

// Column passes (gpslam_hip_marginals_keep_closure_columns): the kept Z = A^-1 U^T is what k_mg_clo_finish's tiles want -- rows of
// mg_ldz(nc) doubles (nc rounded up to the 16 columns of a tile), mg_zrows(N, b) of them (the state rows rounded up to a group of
// kMgGroupRows, plus the 16-row tile that holds the halo state); everything outside the N b x nc entries k_mg_keep_z writes stays zero
constexpr int kMgGroupRows = 48;    // three 16-row tiles: 12, 8 or 4 whole states of block size 4, 6 or 12
inline int mg_ldz(int nc) { return (nc + 15) / 16 * 16; }
inline size_t mg_zrows(int N, int b) { return ((size_t)N * b + kMgGroupRows - 1) / kMgGroupRows * kMgGroupRows + 16; }

// The segmented landmark path (gpslam_hip_marginals_on_segments).  Widest fat block served: Sigma_BB of a segment (its two fat blocks,
// 2 NB square, rounded up to the 16 columns of a tile) is staged once per workgroup in LDS by k_mg_fs_finish -- 128 x 130 doubles =
// 130 KB at NB = 64
constexpr int kMgFsMaxNB = 64;
// G = A_s^-1 H[I_s, B_s] overwrites the marginals' own copy of Y: row (state i, coordinate r) -> i b + r, NCP doubles each.  A wave of
// k_mg_fs_finish reads whole 16-row tiles of a 48-row group and the tile behind it: at most 63 rows past the last interior state's
constexpr int kMgFsPadRows = 64;
inline size_t mg_fs_grows(int N, int b) { return (size_t)N * b + kMgFsPadRows; }
inline int mg_fs_ldz(int NB) { return (2 * NB + 15) / 16 * 16; }
// gather modes of marginals_fs_gather (the three landmark getters)
enum { kMgGatherLmPair = 0, kMgGatherStateLm = 1 };

// What gpslam_hip_marginals leaves on the device.  Only its own methods and the four marginals translation units write it; everything
// else says h->mg.invalidate() where it changes what Sigma depends on (states, landmarks, factors, Qc) -- compile() also h->mg.fit(N)
// -- and reads Z where the pass driver fills it (closures.hip)
struct Marginals {
  bool ok = false;            // the blocks below are those of the handle as it stands
  int N = 0;                  // the N the buffers are sized for
  // the dense path: [P^-1 | U | V] of level 0, Sigma_{i,i}, Sigma_{i,i+1}, the levels above 0 (MgLevels), K, Sigma_LL, Sigma_xL
  DevBuf fac, S, Sn, up, K, Slm, Sxl;
  // gpslam_hip_marginals_keep_closure_columns: on a handle in column passes (clo.P > 1) the marginals keep Z at every state and the
  // inverse of I + U Z (Minv: mg_ldz(clo.nc) squared)
  bool keep_z = false;
  DevBuf Z, Minv;
  // gpslam_hip_marginals_on_segments: the marginals run on the segmented landmark path (marginals_fs.hip) and keep the fat chain's
  // selected inverse (fsD: K blocks Sigma_{k,k}; fsP: one block Sigma_{left,right} per link of the cyclic reduction, the first K - 1 of
  // them Sigma_{k,k+1}) and G at every interior state (mg_fs_grows(N, b) rows of NCP doubles)
  bool on_segments = false;
  DevBuf fsD, fsP, G;
  // gpslam_hip_marginals_keep_pair_terms: the marginals copy Y = [W | Z] -- columns 1 .. R - 1 of the level-0 solution, which later
  // calls may rewrite -- into Y (N x Ym x b doubles; in column passes only the nl landmark columns W) for the pair getters
  // (marginals_pairs.hip); pairs_ok: the last gpslam_hip_marginals left what gpslam_hip_get_state_pair_marginals needs
  bool keep_pairs = false, pairs_ok = false;
  int Ym = 0;
  DevBuf Y;

  void invalidate() { ok = false; pairs_ok = false; }
  // frees every buffer now (they are sized by N, and a handle may live long after its last marginals); the opt-ins stay
  void release_all() {
    Marginals fresh;
    fresh.keep_z = keep_z; fresh.on_segments = on_segments; fresh.keep_pairs = keep_pairs;
    *this = std::move(fresh);
  }
  // the buffers serve n states from here on: another N frees what is there
  void fit(int n) {
    if (N != n) release_all();
    N = n;
  }
};

}  // namespace gps

// the refusals and the staleness rule of every marginals getter (marginals.hip)
int marginals_getter_check(gpslam_hip_handle *h);
// behind the last kernel of gpslam_hip_marginals on either path: reads the pivot flag (the stream is drained), GPSLAM_E_NOT_SPD if a
// pivot was not positive, else the marginals are current (marginals.hip)
int marginals_finish_flag(gpslam_hip_handle *h);
// the closure term of the marginals on a handle in column passes (marginals_clo.hip)
int marginals_closure_term(gpslam_hip_handle *h);
// the marginals of a handle on the segmented landmark path, and the gather behind the landmark getters (marginals_fs.hip)
int marginals_fs(gpslam_hip_handle *h);
int marginals_fs_gather(gpslam_hip_handle *h, int mode, int32_t count, const int32_t *a, const int32_t *b, double *out);
// behind gpslam_hip_marginals' last kernel: the copy of Y for the pair getters (marginals_pairs.hip; nothing without the opt-in)
int marginals_pairs_keep(gpslam_hip_handle *h);
