// marginals_fs.hip -- gpslam_hip_marginals on the segmented landmark path (fatsep.hpp; gpslam_hip_marginals_on_segments): the selected
// inversion through the nested dissection.  I: interior states, F: fat variables (cut states and all landmarks); H_II is block diagonal
// over the segments (A_s = L L^T along the chain, k_fs_factor), S = H_FF - H_FI H_II^-1 H_IF the block-tridiagonal fat chain.
//   (a) the forward half at lambda = 0 (fatsep.hip: fs_forward with y_own: the solver's own launches, the sweep in its two-launch form
//       into the marginals' own Y): fac = [W | E], Y = L^-1 H[I_s, B_s], and per eliminated fat block m its factor L_m (Dfat),
//       P = L_m^-1 H(m,l) (link) and Q = L_m^-1 H(m,r) (Qbuf);
//   (b) Sigma_FF = S^-1, blocks Sigma_{k,k} and Sigma_{k,k+1}: the top block's inverse (k_mg_fs_top), then the cyclic-reduction levels
//       in reverse, one workgroup per eliminated block (k_mg_fs_level): with U = P S_ll + Q S_rl, V = P S_lr + Q S_rr,
//           S_ml = -L_m^-T U,  S_mr = -L_m^-T V,  S_mm = (L_m^-T - S_ml P^T - S_mr Q^T) L_m^-1.
//       Adjacent pairs live in one buffer indexed by the LINK of the pair (mg.fsP[lk] = Sigma_{left,right}): the pair (l, r) of the
//       level above is the link the elimination of m created, (l, m) and (m, r) are the links it consumed; links 0 .. K-2 are the
//       chain's own, so the wanted Sigma_{k,k+1} end up in the first K - 1 blocks;
//   (c) one backward walk per segment (k_mg_fs_walk): G_j = W_j^T (Y_j - E_j G_{j+1}) over Y in place (G = A_s^-1 H[I_s, B_s]; Y carries
//       H's own sign, see k_fs_fat_assemble: "direct terms - Schur complements"), and Takahashi's recurrence for A_s^-1 beside it:
//       Z_jj = W_j^T W_j + M_j Z_{j+1,j+1} M_j^T, Z_{j,j+1} = -M_j Z_{j+1,j+1}, M_j = W_j^T E_j, straight into mg.S / mg.Sn;
//   (d) Sigma_ii += T_i G_i^T, Sigma_{i,i+1} += T_i G_{i+1}^T, T_i = G_i Sigma_BB(s) on v_mfma_f64_16x16x4_f64 (k_mg_fs_finish, the tiles of
//       k_mg_clo_finish with a right operand per segment); the cut states and the two state pairs at every cut from Sigma_{i,F} = -T_i
//       (k_mg_fs_cuts);
//   (e) Sigma_{i,F} is not stored (N b x nl: 80 GB at config 4): the getters gather what they are asked for from G and Sigma_FF
//       (k_mg_fs_gather).
// fp64 only; no atomics, one owner per output entry, every sum in a fixed order: two calls give bit-identical blocks.
// tests/marginals_segmented_model.py is the same algebra in numpy.  What is kept is h->mg.fsD, fsP, G; the limits and shapes (kMgFsMaxNB,
// mg_fs_grows, mg_fs_ldz, the gather modes) are marginals.hpp's; the call ends in marginals.hip's marginals_finish_flag.
#include "marginals_dev.hpp"

namespace impl64 {
#include "api_decl.inc"
}

namespace {

typedef double mgf_d4 __attribute__((ext_vector_type(4)));
typedef double mgf_d2 __attribute__((ext_vector_type(2)));

// In-place Gauss-Jordan inverse without pivoting of the n x n matrix S (row stride ls, LDS), the whole workgroup: every entry owned
// by one thread between two barriers.  The pivots of an SPD matrix are its leading Schur complements (a non-positive one raises the
// flag); a lower-triangular matrix stays lower triangular and its pivots are its diagonal.  (k_mg_clo_inverse of marginals_clo.hip
// has the same steps written out for its constant thread count: see there.)
__device__ inline void mgf_gj_inverse(double *S, int n, int ls, double *colk, double *rowk, int *flag) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int k = 0; k < n; k++) {
    double piv = S[k * ls + k];
    if (!(piv > 0.0)) { if (flag && tid == 0) *flag = 1; piv = 1.0; }
    const double pinv = 1.0 / piv;
    for (int t = tid; t < n; t += nt) { colk[t] = S[t * ls + k]; rowk[t] = S[k * ls + t]; }
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += nt) {
      const int i = idx / n, j = idx - i * n;
      double v;
      if (i == k) v = (j == k) ? pinv : rowk[j] * pinv;
      else if (j == k) v = -colk[i] * pinv;
      else v = S[i * ls + j] - colk[i] * rowk[j] * pinv;
      S[i * ls + j] = v;
    }
    __syncthreads();
  }
}

// the fat chain after the forward half, and its selected inverse
struct MgFsChain {
  const double *Dfat, *link, *Qbuf;   // L_m (the top block: the reduced block itself), P by link, Q by block
  double *SD, *SP;                    // Sigma_{k,k} by block, Sigma_{left,right} by link
  int NB;
  int *flag;
};
constexpr int kMgFsThreads = 256;
constexpr int kMgFsNE = kMgFsMaxNB * kMgFsMaxNB / kMgFsThreads;   // entries of an NB x NB block per thread

// the top of the cyclic reduction: Sigma = D^-1 (symmetrised)
inline size_t mg_fs_top_lds(int NB) { return ((size_t)NB * (NB + 1) + 2 * (size_t)NB) * sizeof(double); }
__global__ void __launch_bounds__(kMgFsThreads) k_mg_fs_top(MgFsChain a, int top) {
  extern __shared__ double mgf_lds[];
  const int NB = a.NB, ls = NB + 1, NB2 = NB * NB, tid = threadIdx.x;
  double *S = mgf_lds, *colk = S + (size_t)NB * ls, *rowk = colk + NB;
  for (int idx = tid; idx < NB2; idx += kMgFsThreads) S[(idx / NB) * ls + idx % NB] = a.Dfat[(size_t)top * NB2 + idx];
  __syncthreads();
  mgf_gj_inverse(S, NB, ls, colk, rowk, a.flag);
  for (int idx = tid; idx < NB2; idx += kMgFsThreads) {
    const int i = idx / NB, j = idx - i * NB;
    a.SD[(size_t)top * NB2 + idx] = 0.5 * (S[i * ls + j] + S[j * ls + i]);
  }
}

// one level back down: block m between l and r (r < 0 at the chain's end).  LDS: W = L_m^-1, then U / V, S_ml / S_mr, T and S_mm in turn
// (3 NB^2 + 2 NB doubles, 97 KB at NB = 64); P, Q and the neighbours' blocks are read where they lie (L2).  Latency-bound like the
// elimination it mirrors: one workgroup per block, a handful of barriers, NB Gauss-Jordan steps for W.
inline size_t mg_fs_level_lds(int NB) { return (3 * (size_t)NB * NB + 2 * (size_t)NB) * sizeof(double); }
__global__ void __launch_bounds__(kMgFsThreads) k_mg_fs_level(MgFsChain a, FatLevel lv) {
  extern __shared__ double mgf_lds[];
  const int NB = a.NB, NB2 = NB * NB, tid = threadIdx.x;
  double *Ws = mgf_lds, *Us = Ws + NB2, *Vs = Us + NB2, *colk = Vs + NB2, *rowk = colk + NB;
  const int *e = lv.elim + 6 * blockIdx.x;
  const int m = e[0], l = e[1], r = e[2], lk_lm = e[3], lk_mr = e[4], lk_new = e[5];
  const bool hr = r >= 0;
  const double *P = a.link + (size_t)lk_lm * NB2, *Q = a.Qbuf + (size_t)m * NB2;
  const double *Sll = a.SD + (size_t)l * NB2, *Srr = hr ? a.SD + (size_t)r * NB2 : Sll, *Slr = hr ? a.SP + (size_t)lk_new * NB2 : Sll;
  for (int idx = tid; idx < NB2; idx += kMgFsThreads) Ws[idx] = a.Dfat[(size_t)m * NB2 + idx];
  __syncthreads();
  mgf_gj_inverse(Ws, NB, NB, colk, rowk, nullptr);   // (a bad pivot was flagged by the elimination that formed L_m)
  double u[kMgFsNE], v[kMgFsNE];
  // U = P S_ll + Q S_rl,  V = P S_lr + Q S_rr
#pragma unroll
  for (int t = 0; t < kMgFsNE; t++) {
    const int idx = tid + kMgFsThreads * t;
    if (idx < NB2) {
      const int i = idx / NB, j = idx - i * NB;
      double au = 0.0, av = 0.0;
      for (int k = 0; k < NB; k++) {
        const double p = P[i * NB + k];
        au = fma(p, Sll[k * NB + j], au);
        if (hr) {
          const double q = Q[i * NB + k];
          au = fma(q, Slr[j * NB + k], au);
          av = fma(p, Slr[k * NB + j], av);
          av = fma(q, Srr[k * NB + j], av);
        }
      }
      Us[idx] = au;
      Vs[idx] = av;
    }
  }
  __syncthreads();
  // S_ml = -W^T U,  S_mr = -W^T V  (W lower triangular)
#pragma unroll
  for (int t = 0; t < kMgFsNE; t++) {
    const int idx = tid + kMgFsThreads * t;
    u[t] = v[t] = 0.0;
    if (idx < NB2) {
      const int i = idx / NB, j = idx - i * NB;
      double au = 0.0, av = 0.0;
      for (int k = i; k < NB; k++) {
        const double w = Ws[k * NB + i];
        au = fma(-w, Us[k * NB + j], au);
        av = fma(-w, Vs[k * NB + j], av);
      }
      u[t] = au;
      v[t] = av;
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < kMgFsNE; t++) {
    const int idx = tid + kMgFsThreads * t;
    if (idx < NB2) {
      const int i = idx / NB, j = idx - i * NB;
      Us[idx] = u[t];
      Vs[idx] = v[t];
      a.SP[(size_t)lk_lm * NB2 + (size_t)j * NB + i] = u[t];          // Sigma_{l,m} = S_ml^T
      if (hr) a.SP[(size_t)lk_mr * NB2 + idx] = v[t];                 // Sigma_{m,r}
    }
  }
  __syncthreads();
  // T = W^T - S_ml P^T - S_mr Q^T
#pragma unroll
  for (int t = 0; t < kMgFsNE; t++) {
    const int idx = tid + kMgFsThreads * t;
    u[t] = 0.0;
    if (idx < NB2) {
      const int i = idx / NB, j = idx - i * NB;
      double acc = Ws[j * NB + i];
      for (int k = 0; k < NB; k++) {
        acc = fma(-Us[i * NB + k], P[j * NB + k], acc);
        if (hr) acc = fma(-Vs[i * NB + k], Q[j * NB + k], acc);
      }
      u[t] = acc;
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < kMgFsNE; t++) {
    const int idx = tid + kMgFsThreads * t;
    if (idx < NB2) Us[idx] = u[t];
  }
  __syncthreads();
  // S_mm = T W, symmetrised
#pragma unroll
  for (int t = 0; t < kMgFsNE; t++) {
    const int idx = tid + kMgFsThreads * t;
    if (idx < NB2) {
      const int i = idx / NB, j = idx - i * NB;
      double acc = 0.0;
      for (int k = j; k < NB; k++) acc = fma(Us[i * NB + k], Ws[k * NB + j], acc);
      Vs[idx] = acc;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < NB2; idx += kMgFsThreads) {
    const int i = idx / NB, j = idx - i * NB;
    a.SD[(size_t)m * NB2 + idx] = 0.5 * (Vs[i * NB + j] + Vs[j * NB + i]);
  }
}

// the segments
struct MgFsSeg {
  const int *cuts;
  const double *fac;            // N x 2 B^2: [W | E]
  double *G;                    // Y on entry of the walk, G behind it: rows i B + r of NCP doubles
  double *Sd, *Sn;              // mg.S, mg.Sn
  const double *SD, *SP;
  int N, K, NB, NCP;
  int pad0, npad;
};

// (c) one workgroup per segment, one thread per border column (2 NB of them over the workgroup's waves; the columns are independent,
// [W | E] of the current state goes through LDS once for all of them); the B x B recurrences of Z ride along on the same threads.
// The columns 2 NB .. NCP - 1 (Y's right-hand side, padding) are zeroed: k_mg_fs_finish multiplies whole tiles.
template <int B> __global__ void __launch_bounds__(256) k_mg_fs_walk(MgFsSeg a) {
  constexpr int BB = B * B, NZ = (BB + 63) / 64;      // (the workgroup has at least 64 threads)
  __shared__ double Fs[2 * BB], Zp[BB], Mm[BB], Zn[BB];
  const int seg = blockIdx.x, c = threadIdx.x, nt = blockDim.x;
  const int j0 = a.cuts[seg] + 1, n = a.cuts[seg + 1] - a.cuts[seg] - 1;
  if (n <= 0) return;
  const int NCP = a.NCP;
  const bool col = c < 2 * a.NB, zcol = !col && c < NCP;
  const double *W = Fs, *E = Fs + BB;
  double g[B];
#pragma unroll
  for (int r = 0; r < B; r++) g[r] = 0.0;
  for (int jj = n - 1; jj >= 0; jj--) {
    const int s = j0 + jj;
    const bool last = jj == n - 1;                    // E of the last interior state couples to the cut, not to an interior state
    for (int k = c; k < 2 * BB; k += nt) Fs[k] = a.fac[(size_t)s * 2 * BB + k];
    __syncthreads();
    double *yp = a.G + (size_t)s * B * NCP + c;
    if (col) {
      double y[B];
#pragma unroll
      for (int r = 0; r < B; r++) y[r] = yp[(size_t)r * NCP];
      if (!last) {
#pragma unroll
        for (int r = 0; r < B; r++)
#pragma unroll
          for (int k = 0; k < B; k++) y[r] = fma(-E[r * B + k], g[k], y[r]);
      }
#pragma unroll
      for (int r = 0; r < B; r++) {
        double acc = 0.0;
#pragma unroll
        for (int k = r; k < B; k++) acc = fma(W[k * B + r], y[k], acc);     // W^T y, W lower triangular
        g[r] = acc;
      }
#pragma unroll
      for (int r = 0; r < B; r++) yp[(size_t)r * NCP] = g[r];
    } else if (zcol) {
#pragma unroll
      for (int r = 0; r < B; r++) yp[(size_t)r * NCP] = 0.0;
    }
    double zd[NZ], zn[NZ];
#pragma unroll
    for (int t = 0; t < NZ; t++) zd[t] = zn[t] = 0.0;
    if (!last) {
      for (int e = c; e < BB; e += nt) {              // M = W^T E
        const int r = e / B, cc = e - r * B;
        double acc = 0.0;
        for (int k = r; k < B; k++) acc = fma(W[k * B + r], E[k * B + cc], acc);
        Mm[e] = acc;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < NZ; t++) {                  // Z_{j,j+1} = -M Z_{j+1,j+1}
        const int e = c + nt * t;
        if (e < BB) {
          const int r = e / B, cc = e - r * B;
          double acc = 0.0;
          for (int k = 0; k < B; k++) acc = fma(-Mm[r * B + k], Zp[k * B + cc], acc);
          zn[t] = acc;
          Zn[e] = acc;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < NZ; t++) {                    // Z_jj = W^T W - Z_{j,j+1} M^T
      const int e = c + nt * t;
      if (e < BB) {
        const int r = e / B, cc = e - r * B;
        double acc = 0.0;
        for (int k = max(r, cc); k < B; k++) acc = fma(W[k * B + r], W[k * B + cc], acc);
        if (!last)
          for (int k = 0; k < B; k++) acc = fma(-Zn[r * B + k], Mm[cc * B + k], acc);
        zd[t] = acc;
      }
    }
    __syncthreads();                                  // (the last readers of Zp were in front of the previous barrier; this one is for Fs)
#pragma unroll
    for (int t = 0; t < NZ; t++) {
      const int e = c + nt * t;
      if (e < BB) {
        Zp[e] = zd[t];
        a.Sd[(size_t)s * BB + e] = zd[t];
        a.Sn[(size_t)s * BB + e] = zn[t];             // (the last interior state's pair with the cut: k_mg_fs_cuts)
      }
    }
    __syncthreads();
  }
}

// (d) Sigma_{i,i} += T_i G_i^T, Sigma_{i,i+1} += T_i G_{i+1}^T, T_i = G_i Sigma_BB(s): k_mg_clo_finish's tiles (marginals_clo.hip has the
// operand layouts) with one workgroup per segment.  Sigma_BB(s) = [S_ss S_s,s+1; . S_s+1,s+1] is staged once in LDS, zero-padded to ldz =
// 2 NB rounded up to 16 (ldz (ldz + 2) doubles, 130 KB at NB = 64), its rows permuted inside each group of 16 so that the accumulator
// tiles of T^T = Sigma_BB G_t^T are the A operand of out = T G_u^T as they stand.  A wave owns groups of 48 rows of G (whole states,
// three 16-row tiles) of its segment and reads the tile behind a group for the halo state; rows past the segment's last interior
// state belong to the cut (zero) or to the next segment and are masked at the store.  One owner per entry, fixed order, no atomics.
constexpr int kMgFsWaves = 8, kMgFsGroupRows = 48;
inline size_t mg_fs_finish_lds(int ldz) { return (size_t)ldz * (ldz + 2) * sizeof(double); }
template <int B> __global__ void __launch_bounds__(64 * kMgFsWaves) k_mg_fs_finish(MgFsSeg a) {
  static_assert(kMgFsGroupRows % B == 0 && kMgFsGroupRows % 16 == 0, "a group is whole states and whole tiles");
  extern __shared__ double mgf_lds[];
  constexpr int BB = B * B, NTMAX = 2 * kMgFsMaxNB / 16;
  const int seg = blockIdx.x, tid = threadIdx.x;
  const int j0 = a.cuts[seg] + 1, n = a.cuts[seg + 1] - a.cuts[seg] - 1;
  if (n <= 0) return;
  const int NB = a.NB, NB2 = NB * NB, NCP = a.NCP, ldz = (2 * NB + 15) / 16 * 16, ls = ldz + 2, nt = ldz / 16;
  {
    const double *D0 = a.SD + (size_t)seg * NB2, *D1 = a.SD + (size_t)(seg + 1) * NB2, *P01 = a.SP + (size_t)seg * NB2;
    for (int idx = tid; idx < ldz * ldz; idx += 64 * kMgFsWaves) {
      const int row = idx / ldz, cc = idx - row * ldz, x = row & 15;
      const int src = (row & ~15) + 4 * (x & 3) + (x >> 2);
      double v = 0.0;
      if (src < 2 * NB && cc < 2 * NB) {
        const bool bu = src >= NB, bv = cc >= NB;
        const int uu = src - (bu ? NB : 0), vv = cc - (bv ? NB : 0);
        v = bu ? (bv ? D1[uu * NB + vv] : P01[vv * NB + uu]) : (bv ? P01[uu * NB + vv] : D0[uu * NB + vv]);
      }
      mgf_lds[(size_t)row * ls + cc] = v;
    }
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const size_t slast = (size_t)(j0 + n - 1);
  const int ngroups = (n * B + kMgFsGroupRows - 1) / kMgFsGroupRows;
  for (int grp = wave; grp < ngroups; grp += kMgFsWaves) {
    const size_t row0 = (size_t)j0 * B + (size_t)grp * kMgFsGroupRows;
#pragma unroll
    for (int t = 0; t < kMgFsGroupRows / 16; t++) {
      mgf_d4 acc[NTMAX];
#pragma unroll
      for (int ct = 0; ct < NTMAX; ct++) acc[ct] = mgf_d4{0.0, 0.0, 0.0, 0.0};
      const double *zt = a.G + (row0 + 16 * t + r) * NCP + 4 * q;
      const double *mrow = mgf_lds + (size_t)r * ls + 4 * q;
#pragma unroll 2
      for (int kt = 0; kt < nt; kt++) {
        const mgf_d4 z = *reinterpret_cast<const mgf_d4 *>(zt + 16 * kt);
#pragma unroll
        for (int ct = 0; ct < NTMAX; ct++) {
          if (ct < nt) {                                     // (wave-uniform)
            const double *mp = mrow + (size_t)16 * ct * ls + 16 * kt;
            const mgf_d2 m0 = *reinterpret_cast<const mgf_d2 *>(mp), m1 = *reinterpret_cast<const mgf_d2 *>(mp + 2);
            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(m0.x, z.x, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(m0.y, z.y, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(m1.x, z.z, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(m1.y, z.w, acc[ct], 0, 0, 0);
          }
        }
      }
      // the column tiles that hold the states of rows 16 t .. 16 t + 15 and the successor of the last of them
      const int ulo = (B * ((16 * t) / B)) / 16, uhi = min(kMgFsGroupRows / 16, (B * ((16 * t + 15) / B + 2) - 1) / 16);
      for (int u = ulo; u <= uhi; u++) {
        mgf_d4 out = mgf_d4{0.0, 0.0, 0.0, 0.0};
        const double *zu = a.G + (row0 + 16 * u + r) * NCP + 4 * q;
#pragma unroll
        for (int ct = 0; ct < NTMAX; ct++) {
          if (ct < nt) {
            const mgf_d4 z = *reinterpret_cast<const mgf_d4 *>(zu + 16 * ct);
            out = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[ct].x, z.x, out, 0, 0, 0);
            out = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[ct].y, z.y, out, 0, 0, 0);
            out = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[ct].z, z.z, out, 0, 0, 0);
            out = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[ct].w, z.w, out, 0, 0, 0);
          }
        }
        const size_t hh = row0 + 16 * u + r;
        const size_t i2 = hh / B;
        const int cc = (int)(hh - i2 * B);
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
          const size_t g = row0 + 16 * t + q + 4 * jj;
          const size_t i = g / B;
          const int rr = (int)(g - i * B);
          if (i <= slast && i2 <= slast) {
            if (i2 == i) a.Sd[i * BB + rr * B + cc] += out[jj];
            else if (i2 == i + 1) a.Sn[i * BB + rr * B + cc] += out[jj];
          }
        }
      }
    }
  }
}

// the cut states and the state pairs at every cut, one wave per cut k (state `cut`): Sigma_{cut,cut} = S_kk[0:B, 0:B];
// Sigma_{cut,cut+1} = -(G_{cut+1} Sigma_BB(k)[:, 0:B])^T, or S_{k,k+1}[0:B, 0:B] where the next state is a cut as well (zero behind the last
// state); Sigma_{cut-1,cut} = -G_{cut-1} Sigma_BB(k-1)[:, NB:NB+B] where cut - 1 is an interior state.  Then the coordinates that are no
// variable (ROT3_BIAS's pads) report zero rows and columns on every state, as k_mg_finish has it (k_mg_fs_pads).
template <int B> __global__ void __launch_bounds__(64) k_mg_fs_cuts(MgFsSeg a) {
  constexpr int BB = B * B;
  const int k = blockIdx.x, lane = threadIdx.x, NB = a.NB, NB2 = NB * NB, NCP = a.NCP;
  const int cut = a.cuts[k];
  const double *D = a.SD + (size_t)k * NB2;
  for (int e = lane; e < BB; e += 64) {
    const int r = e / B, c = e - r * B;
    a.Sd[(size_t)cut * BB + e] = D[r * NB + c];
    double v = 0.0;
    if (k < a.K - 1) {
      const double *Pk = a.SP + (size_t)k * NB2;
      if (a.cuts[k + 1] == cut + 1) v = Pk[r * NB + c];
      else {
        const double *g = a.G + ((size_t)(cut + 1) * B + c) * NCP;
        double acc = 0.0;
        for (int q = 0; q < NB; q++) acc = fma(g[q], D[q * NB + r], acc);
        for (int q = 0; q < NB; q++) acc = fma(g[NB + q], Pk[r * NB + q], acc);
        v = -acc;
      }
    }
    a.Sn[(size_t)cut * BB + e] = v;
    if (k > 0 && a.cuts[k - 1] < cut - 1) {
      const double *Pm = a.SP + (size_t)(k - 1) * NB2;
      const double *g = a.G + ((size_t)(cut - 1) * B + r) * NCP;
      double acc = 0.0;
      for (int q = 0; q < NB; q++) acc = fma(g[q], Pm[q * NB + c], acc);
      for (int q = 0; q < NB; q++) acc = fma(g[NB + q], D[q * NB + c], acc);
      a.Sn[(size_t)(cut - 1) * BB + e] = -acc;
    }
  }
}
template <int B> __global__ void __launch_bounds__(256) k_mg_fs_pads(MgFsSeg a) {
  constexpr int BB = B * B;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)a.N * BB) return;
  const int e = (int)(t % BB), r = e / B, c = e - r * B;
  if ((r >= a.pad0 && r < a.pad0 + a.npad) || (c >= a.pad0 && c < a.pad0 + a.npad)) { a.Sd[t] = 0.0; a.Sn[t] = 0.0; }
}

// (e) the landmark getters, one thread per output entry.  Item t: (a[t], b[t]) = two landmarks (kMgGatherLmPair: ld x ld) or a state and a
// landmark (kMgGatherStateLm: b x ld).  Dense border: entries of S_lm / S_x_lm.  Segmented: entries of Sigma_FF where both ends are fat
// variables, and -G_i Sigma_BB(s)[:, the landmark's columns] for an interior state i of segment s.  The host has checked that the blocks
// are the same or neighbours.
struct MgFsGather {
  int mode, dense, count, B, ld, nl, NB, NCP;
  const int *a, *b, *segid, *lm_fat, *lm_slot;
  const double *SD, *SP, *G, *Slm, *Sxl;
  int pad0, npad;
  double *out;
};
__device__ inline double mgf_fat_entry(const MgFsGather &g, int ka, int ra, int kb, int rb) {
  const size_t NB2 = (size_t)g.NB * g.NB;
  if (ka == kb) return g.SD[ka * NB2 + (size_t)ra * g.NB + rb];
  if (kb == ka + 1) return g.SP[ka * NB2 + (size_t)ra * g.NB + rb];
  return g.SP[kb * NB2 + (size_t)rb * g.NB + ra];
}
__global__ void __launch_bounds__(256) k_mg_fs_gather(MgFsGather g) {
  const int rows = g.mode == kMgGatherStateLm ? g.B : g.ld, per = rows * g.ld;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)g.count * per) return;
  const int item = (int)(t / per), e = (int)(t - (size_t)item * per), p = e / g.ld, q = e - p * g.ld;
  const int ia = g.a[item], lb = g.b[item];
  double v;
  if (g.dense) {
    v = g.mode == kMgGatherStateLm ? g.Sxl[((size_t)ia * g.B + p) * g.nl + (size_t)lb * g.ld + q]
                                   : g.Slm[((size_t)ia * g.ld + p) * g.nl + (size_t)lb * g.ld + q];
  } else {
    const int kb = g.lm_fat[lb], rb = g.B + g.lm_slot[lb] * g.ld + q;
    if (g.mode == kMgGatherLmPair) v = mgf_fat_entry(g, g.lm_fat[ia], g.B + g.lm_slot[ia] * g.ld + p, kb, rb);
    else {
      const int sg = g.segid[ia];
      if (sg < 0) v = mgf_fat_entry(g, -1 - sg, p, kb, rb);
      else {
        const double *gi = g.G + ((size_t)ia * g.B + p) * g.NCP;
        double acc = 0.0;
        for (int u = 0; u < g.NB; u++) acc = fma(gi[u], mgf_fat_entry(g, sg, u, kb, rb), acc);
        for (int u = 0; u < g.NB; u++) acc = fma(gi[g.NB + u], mgf_fat_entry(g, sg + 1, u, kb, rb), acc);
        v = -acc;
      }
      if (p >= g.pad0 && p < g.pad0 + g.npad) v = 0.0;
    }
  }
  g.out[t] = v;
}

}  // namespace

int marginals_fs(gpslam_hip_handle *h) {
  FatSepPlan &p = h->fs;
  const int N = h->N, B = h->b, BB = B * B, K = p.K, NB = p.NB, NCP = p.NCP;
  if (NB > kMgFsMaxNB) {
    char msg[200];
    snprintf(msg, sizeof msg, "marginals on the segmented landmark path: fat blocks of NB = %d columns are wider than the limit of %d", NB, kMgFsMaxNB);
    return fail(h, GPSLAM_E_UNSUPPORTED, msg);
  }
  h->mg.fit(N);
  const size_t NB2 = (size_t)NB * NB, gbytes = mg_fs_grows(N, B) * NCP * sizeof(double);
  HIPCHK(h->mg.S.reserve((size_t)N * BB * sizeof(double)));
  HIPCHK(h->mg.Sn.reserve((size_t)N * BB * sizeof(double)));
  HIPCHK(h->mg.fsD.reserve((size_t)K * NB2 * sizeof(double)));
  HIPCHK(h->mg.fsP.reserve((size_t)p.nlinks * NB2 * sizeof(double)));
  HIPCHK(h->mg.G.reserve(gbytes));
  hipStream_t st = h->stream;
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), st));
  // Y is zero wherever the sweep does not write (columns before their first right-hand side, padding, the cut states' rows); G is not
  HIPCHK(hipMemsetAsync(h->mg.G.p, 0, gbytes, st));
  int rc;
  if ((rc = impl64::launch_factors(h, LaunchMode{}, 0, 0)) || (rc = impl64::launch_assemble(h, LaunchMode{}, false))) return rc;
  if ((rc = fs_forward(h, 0.0, h->mg.G.as<double>()))) return rc;
  MgFsChain c;
  c.Dfat = p.Dfat.as<double>(); c.link = p.link.as<double>(); c.Qbuf = p.Qbuf.as<double>();
  c.SD = h->mg.fsD.as<double>(); c.SP = h->mg.fsP.as<double>(); c.NB = NB; c.flag = h->flag.as<int>();
  // (process-wide per kernel: always the size of the widest block, whatever this handle's)
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mg_fs_level), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mg_fs_level_lds(kMgFsMaxNB)));
  k_mg_fs_top<<<dim3(1), dim3(kMgFsThreads), mg_fs_top_lds(NB), st>>>(c, p.top);
  for (int li = (int)p.levels.size() - 1; li >= 0; li--) {
    const FatLevel fl = fat_level(p.levels[li], p.d_elim);
    k_mg_fs_level<<<dim3(fl.nelim), dim3(kMgFsThreads), mg_fs_level_lds(NB), st>>>(c, fl);
  }
  HIPCHK(hipGetLastError());
  MgFsSeg s;
  s.cuts = p.d_cuts.as<int>(); s.fac = p.fac.as<double>(); s.G = h->mg.G.as<double>();
  s.Sd = h->mg.S.as<double>(); s.Sn = h->mg.Sn.as<double>(); s.SD = c.SD; s.SP = c.SP;
  s.N = N; s.K = K; s.NB = NB; s.NCP = NCP;
  const MgPads pads = mg_pads(h);
  s.pad0 = pads.pad0; s.npad = pads.npad;
  const int nseg = K - 1, walk_threads = (NCP + 63) / 64 * 64, ldz = mg_fs_ldz(NB);
  hipError_t ea = hipSuccess;
  dispatch_b(B, [&](auto tag) {
    constexpr int BV = decltype(tag)::value;
    ea = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mg_fs_finish<BV>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)mg_fs_finish_lds(mg_fs_ldz(kMgFsMaxNB)));
    if (ea != hipSuccess) return;
    if (nseg > 0) {
      k_mg_fs_walk<BV><<<dim3(nseg), dim3(walk_threads), 0, st>>>(s);
      k_mg_fs_finish<BV><<<dim3(nseg), dim3(64 * kMgFsWaves), mg_fs_finish_lds(ldz), st>>>(s);
    }
    k_mg_fs_cuts<BV><<<dim3(K), dim3(64), 0, st>>>(s);
    if (pads.npad > 0) k_mg_fs_pads<BV><<<dim3((unsigned)(((size_t)N * BB + 255) / 256)), dim3(256), 0, st>>>(s);
  });
  HIPCHK(ea);
  HIPCHK(hipGetLastError());
  return marginals_finish_flag(h);
}

// the three landmark getters (marginals.hip has checked refusals, staleness and pointers)
int marginals_fs_gather(gpslam_hip_handle *h, int mode, int32_t count, const int32_t *a, const int32_t *b, double *out) {
  if (count == 0) return 0;
  const FatSepPlan &p = h->fs;
  const bool seg = p.active, state = mode == kMgGatherStateLm;
  const char *who = state ? "get_state_landmark_marginals" : "get_landmark_pair_marginals";
  char msg[256];
  for (int t = 0; t < count; t++) {
    if (a[t] < 0 || a[t] >= (state ? h->N : h->L) || b[t] < 0 || b[t] >= h->L) {
      snprintf(msg, sizeof msg, "%s: item %d (%d, %d) is out of range", who, t, a[t], b[t]);
      return fail(h, GPSLAM_E_INVALID, msg);
    }
    if (!seg) continue;
    const int kb = p.h_lm_fat[b[t]];
    bool ok;
    if (state) {
      // the state's own fat block or a neighbour of it (a cut state), or one of the two fat blocks of its segment
      const int k = (int)(std::upper_bound(p.cuts.begin(), p.cuts.end(), a[t]) - p.cuts.begin()) - 1;   // cuts[k] <= state
      ok = p.cuts[k] == a[t] ? std::abs(kb - k) <= 1 : (kb == k || kb == k + 1);
      if (!ok) snprintf(msg, sizeof msg, "%s: item %d: landmark %d (fat block %d) is not in a fat block next to state %d's segment", who, t, b[t], kb, a[t]);
    } else {
      ok = std::abs(p.h_lm_fat[a[t]] - kb) <= 1;
      if (!ok) snprintf(msg, sizeof msg, "%s: item %d: landmarks %d and %d are in fat blocks %d and %d, not the same or neighbouring ones", who, t, a[t], b[t], p.h_lm_fat[a[t]], kb);
    }
    if (!ok) return fail(h, GPSLAM_E_INVALID, msg);
  }
  struct { DevBuf a, b, out; } sc;   // this call's own buffers
  int rc;
  std::vector<int> va(a, a + count), vb(b, b + count);
  if ((rc = upload(h, sc.a, va)) || (rc = upload(h, sc.b, vb))) return rc;
  MgFsGather g;
  g.mode = mode; g.dense = seg ? 0 : 1; g.count = count; g.B = h->b; g.ld = h->ld; g.nl = h->nl; g.NB = p.NB; g.NCP = p.NCP;
  g.a = sc.a.as<int>(); g.b = sc.b.as<int>(); g.segid = p.d_segid.as<int>(); g.lm_fat = p.d_lm_fat.as<int>(); g.lm_slot = p.d_lm_slot.as<int>();
  g.SD = h->mg.fsD.as<double>(); g.SP = h->mg.fsP.as<double>(); g.G = h->mg.G.as<double>();
  g.Slm = h->mg.Slm.as<double>(); g.Sxl = h->mg.Sxl.as<double>();
  g.pad0 = mg_pads(h).pad0; g.npad = mg_pads(h).npad;
  const size_t total = (size_t)count * (state ? h->b : h->ld) * h->ld;
  HIPCHK(sc.out.reserve(total * sizeof(double)));
  g.out = sc.out.as<double>();
  k_mg_fs_gather<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream>>>(g);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, sc.out.p, total * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
