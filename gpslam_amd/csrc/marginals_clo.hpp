// marginals_clo.hpp -- what gpslam_hip_marginals on a handle in column passes shares between its translation units (marginals.hip,
// marginals_clo.hip) and the pass driver's launches (closures.hip): the layout of the kept Z and the kernel that fills it
#pragma once

#include "closures.hpp"

namespace gps {

// gpslam_hip_marginals on a handle in column passes: slice p's closure columns of every state's level-0 solution into the kept
// Z (N b rows of ldz doubles, a state row contiguous in the closure index): Z[s b + k][k0 d + q] = x[s][col0 + q][k].
// The buffer is what k_mg_clo_finish's tiles want: rows of mg_ldz(nc) doubles (nc rounded up to the 16 columns of a tile), and
// mg_zrows(N, b) of them (the state rows rounded up to a group of kMgGroupRows, plus the 16-row tile that holds the halo state);
// everything outside the N b x nc entries written here stays zero.
constexpr int kMgGroupRows = 48;    // three 16-row tiles: 12, 8 or 4 whole states of block size 4, 6 or 12
inline int mg_ldz(int nc) { return (nc + 15) / 16 * 16; }
inline size_t mg_zrows(int N, int b) { return ((size_t)N * b + kMgGroupRows - 1) / kMgGroupRows * kMgGroupRows + 16; }
template <int d> __global__ void __launch_bounds__(256) k_mg_keep_z(CloArgs a, CloPass p, double *Z, int ldz) {
  const int w = (p.k1 - p.k0) * d, per = w * a.B;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)a.N * per) return;
  const size_t s = i / per;
  const int u = (int)(i - s * per), q = u / a.B, k = u - q * a.B;
  Z[(s * a.B + k) * ldz + p.k0 * d + q] = a.x[(s * a.R + a.col0 + q) * a.B + k];
}

}  // namespace gps
