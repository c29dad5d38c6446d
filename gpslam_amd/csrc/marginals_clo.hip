// marginals_clo.hip -- gpslam_hip_marginals on a handle whose loop closures go through the solver in column passes
// (gpslam_hip_marginals_keep_closure_columns; marginals.hip (c), api_impl.inc launch_solve_passes with keep_z): the closure term
//   Sigma_{i,i} -= Z_i M^-1 Z_i^T,   Sigma_{i,i+1} -= Z_i M^-1 Z_{i+1}^T,   M = I + 1/2 (U Z + (U Z)^T),
// with Z = A^-1 U^T kept at every state (k_mg_keep_z) and nc = closures * d up to kCloWideMax = 120.  A translation unit of its
// own: the kernels of marginals.hip stay what they were, byte for byte.  Z and M^-1 are h->mg.Z, h->mg.Minv; Z's shape (mg_ldz,
// mg_zrows, kMgGroupRows) is marginals.hpp's, the kernel that fills it (k_mg_keep_z, launched by closures.hip) marginals_dev.hpp's.
#include "marginals_dev.hpp"

namespace {

// M = I + 1/2 (U Z + (U Z)^T) from W = U [X | Z] exactly as k_clo_solve_wide forms it, inverted in place in dynamic LDS
// (nc (nc + 1) + 2 nc doubles) by Gauss-Jordan steps without pivoting (a non-positive pivot raises the flag): one
// workgroup of 1024 threads, every entry owned by one thread between two barriers.  The steps are marginals_fs.hip's mgf_gj_inverse with
// the thread count a constant and the flag never null, written out: through the shared function (templated on the thread count,
// the flag assumed non-null) the compiler schedules this kernel differently, and its bytes are kept.  Writes the symmetrised inverse, zero-padded to ldz x ldz.
struct MgCloInv {
  const double *W;              // nc x ldw, U Z in columns nr .. nr + nc - 1
  int ldw, nr, nc, ldz;
  double *Minv;                 // ldz x ldz
  int *flag;
};
inline size_t mg_clo_inverse_lds(int nc) { return ((size_t)nc * (nc + 1) + 2 * (size_t)nc) * sizeof(double); }
constexpr int kMgInvThreads = 1024;   // (16 waves: a step is LDS latency, 256 threads took 10.6 us per step at nc = 120)
__global__ void __launch_bounds__(kMgInvThreads) k_mg_clo_inverse(MgCloInv a) {
  extern __shared__ double mg_lds[];
  const int tid = threadIdx.x, nc = a.nc, ls = nc + 1;
  double *S = mg_lds, *colk = mg_lds + (size_t)nc * ls, *rowk = colk + nc;
  for (int idx = tid; idx < nc * nc; idx += kMgInvThreads) {
    const int i = idx / nc, j = idx - i * nc;
    S[i * ls + j] = clo_sym_entry(i == j, a.W[(size_t)i * a.ldw + a.nr + j], a.W[(size_t)j * a.ldw + a.nr + i]);
  }
  __syncthreads();
  for (int k = 0; k < nc; k++) {
    double piv = S[k * ls + k];
    if (!(piv > 0.0)) { if (tid == 0) *a.flag = 1; piv = 1.0; }
    const double pinv = 1.0 / piv;
    for (int t = tid; t < nc; t += kMgInvThreads) { colk[t] = S[t * ls + k]; rowk[t] = S[k * ls + t]; }
    __syncthreads();
    for (int idx = tid; idx < nc * nc; idx += kMgInvThreads) {
      const int i = idx / nc, j = idx - i * nc;
      double v;
      if (i == k) v = (j == k) ? pinv : rowk[j] * pinv;
      else if (j == k) v = -colk[i] * pinv;
      else v = S[i * ls + j] - colk[i] * rowk[j] * pinv;
      S[i * ls + j] = v;
    }
    __syncthreads();
  }
  for (int idx = tid; idx < a.ldz * a.ldz; idx += kMgInvThreads) {
    const int i = idx / a.ldz, j = idx - i * a.ldz;
    a.Minv[idx] = (i < nc && j < nc) ? 0.5 * (S[i * ls + j] + S[j * ls + i]) : 0.0;
  }
}

// Sigma_{i,i} -= T_i Z_i^T, Sigma_{i,i+1} -= T_i Z_{i+1}^T, T_i = Z_i M^-1: a dense GEMM (N b x nc) (nc x nc) with a resident right
// operand, on v_mfma_f64_16x16x4_f64 (operand layouts: fatsep.hpp, k_fs_syrk).  Z is the kept buffer of k_mg_keep_z: N b rows (state
// i, coordinate r -> row i B + r) of ldz doubles.  M^-1 sits in LDS once per workgroup (ldz (ldz + 2) doubles, 130 KB at nc = 120).
// A wave owns a group of kMgGroupRows = 48 rows -- whole states for every block size, three full 16-row tiles -- and reads the 16
// rows behind it for the halo state (k_mg_keep_z's padding keeps them in bounds and zero behind the last state).  Per row tile t:
//   (1) T^T = M^-1 Z_t^T, nt = ldz / 16 accumulator tiles: the A operand is M^-1 from LDS, the B operand Z_t^T from global memory, a
//       lane (r = lane & 15, q = lane >> 4) reading the four doubles 16 kt + 4 q .. + 3 of its row at once (one 32-byte load: the k
//       index of MFMA step j is 16 kt + 4 q + j on both operands).  LDS row rho of M^-1 holds row (rho & ~15) + pi(rho & 15),
//       pi(x) = 4 (x & 3) + (x >> 2), so that accumulator register j of lane (r, q) is T[g0 + r][16 ct + 4 q + j]: exactly the A
//       operand of step j of
//   (2) out = T Z_u^T for the column tiles u whose states can be the row tile's own or their successors (two or three of four), with
//       the same 32-byte loads of Z_u as B operand: no shuffles, no LDS round trip.  The C layout (col = lane & 15, row = (lane >> 4)
//       + 4 reg) gives every lane four entries; an entry whose column state is the row's own goes to Sigma_{i,i}, the successor's to
//       Sigma_{i,i+1}, everything else is dropped (the tiles' off-band part: the price of full tiles).
// Every output entry has one owner and one summation order: no atomics.  The last state's Sigma_{i,i+1} is not touched.
struct MgCloFinish {
  double *Sd, *Sn;
  const double *Z, *Minv;
  int N, ldz, ngroups;
};
constexpr int kMgCloWaves = 8;
typedef double mg_d4 __attribute__((ext_vector_type(4)));
typedef double mg_d2 __attribute__((ext_vector_type(2)));
inline size_t mg_clo_finish_lds(int ldz) { return (size_t)ldz * (ldz + 2) * sizeof(double); }
template <int B> __global__ void __launch_bounds__(64 * kMgCloWaves) k_mg_clo_finish(MgCloFinish a) {
  static_assert(kMgGroupRows % B == 0 && kMgGroupRows % 16 == 0, "a group is whole states and whole tiles");
  extern __shared__ double mg_lds[];
  constexpr int BB = B * B, NTMAX = kCloWideMax / 16 + 1;
  const int tid = threadIdx.x, ldz = a.ldz, ls = ldz + 2, nt = ldz / 16, half = ldz / 2;
  for (int idx = tid; idx < ldz * half; idx += 64 * kMgCloWaves) {
    const int row = idx / half, c2 = idx - row * half, x = row & 15;
    const int src = (row & ~15) + 4 * (x & 3) + (x >> 2);
    *reinterpret_cast<mg_d2 *>(mg_lds + (size_t)row * ls + 2 * c2) = *reinterpret_cast<const mg_d2 *>(a.Minv + (size_t)src * ldz + 2 * c2);
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  for (int grp = blockIdx.x * kMgCloWaves + wave; grp < a.ngroups; grp += gridDim.x * kMgCloWaves) {
    const size_t row0 = (size_t)grp * kMgGroupRows;
#pragma unroll
    for (int t = 0; t < kMgGroupRows / 16; t++) {
      mg_d4 acc[NTMAX];
#pragma unroll
      for (int ct = 0; ct < NTMAX; ct++) acc[ct] = mg_d4{0.0, 0.0, 0.0, 0.0};
      const double *zt = a.Z + (row0 + 16 * t + r) * ldz + 4 * q;
      const double *mrow = mg_lds + (size_t)r * ls + 4 * q;
#pragma unroll 2
      for (int kt = 0; kt < nt; kt++) {
        const mg_d4 z = *reinterpret_cast<const mg_d4 *>(zt + 16 * kt);
#pragma unroll
        for (int ct = 0; ct < NTMAX; ct++) {
          if (ct < nt) {                                     // (wave-uniform)
            const double *mp = mrow + (size_t)16 * ct * ls + 16 * kt;
            const mg_d2 m0 = *reinterpret_cast<const mg_d2 *>(mp), m1 = *reinterpret_cast<const mg_d2 *>(mp + 2);
            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(m0.x, z.x, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(m0.y, z.y, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(m1.x, z.z, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(m1.y, z.w, acc[ct], 0, 0, 0);
          }
        }
      }
      // the column tiles that hold the states of rows 16 t .. 16 t + 15 and the successor of the last of them
      const int ulo = (B * ((16 * t) / B)) / 16, uhi = min(kMgGroupRows / 16, (B * ((16 * t + 15) / B + 2) - 1) / 16);
      for (int u = ulo; u <= uhi; u++) {
        mg_d4 out = mg_d4{0.0, 0.0, 0.0, 0.0};
        const double *zu = a.Z + (row0 + 16 * u + r) * ldz + 4 * q;
#pragma unroll
        for (int ct = 0; ct < NTMAX; ct++) {
          if (ct < nt) {
            const mg_d4 z = *reinterpret_cast<const mg_d4 *>(zu + 16 * ct);
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
          if (i < (size_t)a.N) {
            if (i2 == i) a.Sd[i * BB + rr * B + cc] -= out[jj];
            else if (i2 == i + 1 && i2 < (size_t)a.N) a.Sn[i * BB + rr * B + cc] -= out[jj];
          }
        }
      }
    }
  }
}

}  // namespace

// behind the column passes of the marginals' launch_solve (W = U [X | Z] in clo.W, Z in mg.Z) and in front of k_mg_finish: M^-1 into mg.Minv, then the term
int marginals_closure_term(gpslam_hip_handle *h) {
  const int N = h->N, B = h->b, ldz = mg_ldz(h->clo.nc);
  MgCloInv ci;
  ci.W = h->clo.W.as<double>(); ci.ldw = clo_ldw(h); ci.nr = 1 + h->nl; ci.nc = h->clo.nc; ci.ldz = ldz;
  ci.Minv = h->mg.Minv.as<double>(); ci.flag = h->flag.as<int>();
  // (process-wide per kernel: always the size of the widest system, whatever this handle's)
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mg_clo_inverse), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)mg_clo_inverse_lds(kCloWideMax)));
  k_mg_clo_inverse<<<dim3(1), dim3(kMgInvThreads), mg_clo_inverse_lds(h->clo.nc), h->stream>>>(ci);
  MgCloFinish cf;
  cf.Sd = h->mg.S.as<double>(); cf.Sn = h->mg.Sn.as<double>(); cf.Z = h->mg.Z.as<double>(); cf.Minv = h->mg.Minv.as<double>();
  cf.N = N; cf.ldz = ldz; cf.ngroups = (int)(((size_t)N * B + kMgGroupRows - 1) / kMgGroupRows);
  const int grid = std::min(nblocks(cf.ngroups, kMgCloWaves), 256);   // (M^-1 is staged once per workgroup: no more of them than CUs)
  hipError_t ea = hipSuccess;
  dispatch_b(B, [&](auto tag) {
    constexpr int BV = decltype(tag)::value;
    ea = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mg_clo_finish<BV>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)mg_clo_finish_lds(mg_ldz(kCloWideMax)));
    if (ea == hipSuccess) k_mg_clo_finish<BV><<<dim3(grid), dim3(64 * kMgCloWaves), mg_clo_finish_lds(ldz), h->stream>>>(cf);
  });
  HIPCHK(ea);
  HIPCHK(hipGetLastError());
  return 0;
}
