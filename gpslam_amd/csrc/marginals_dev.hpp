// marginals_dev.hpp -- the device helpers the marginals' translation units share, one copy of each (behind api_common.hpp: the handle
// is complete here), and the kernel the pass driver launches for them (closures.hip: k_mg_keep_z)
#pragma once

#include "api_common.hpp"

namespace gps {

// the coordinates of a state that are no variable and report zero rows and columns: ROT3_BIAS's three pad components of the velocity slot
struct MgPads { int pad0, npad; };
inline MgPads mg_pads(const gpslam_hip_handle *h) { return h->mf == ROT3_BIAS ? MgPads{9, 3} : MgPads{0, 0}; }

// dst[r][c] = f(r, c) for a B x B row-major matrix in LDS, one wave: every lane evaluates its entries first, then writes them,
// so f may read dst
template <int B, typename F> __device__ inline void mg_set(double *dst, F f) {
  constexpr int NE = (B * B + 63) / 64;
  double v[NE];
#pragma unroll
  for (int t = 0; t < NE; t++) {
    const int e = threadIdx.x + 64 * t;
    v[t] = (e < B * B) ? f(e / B, e % B) : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < NE; t++) {
    const int e = threadIdx.x + 64 * t;
    if (e < B * B) dst[e] = v[t];
  }
  __syncthreads();
}

// gpslam_hip_marginals on a handle in column passes: slice p's closure columns of every state's level-0 solution into the kept
// Z (N b rows of ldz doubles, a state row contiguous in the closure index): Z[s b + k][k0 d + q] = x[s][col0 + q][k]
template <int d> __global__ void __launch_bounds__(256) k_mg_keep_z(CloArgs a, CloPass p, double *Z, int ldz) {
  const int w = (p.k1 - p.k0) * d, per = w * a.B;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)a.N * per) return;
  const size_t s = i / per;
  const int u = (int)(i - s * per), q = u / a.B, k = u - q * a.B;
  Z[(s * a.B + k) * ldz + p.k0 * d + q] = a.x[(s * a.R + a.col0 + q) * a.B + k];
}

}  // namespace gps
