// marginals_fs.hpp -- gpslam_hip_marginals on the segmented landmark path (marginals_fs.hip; gpslam_hip_marginals_on_segments): the
// limits and buffer shapes its translation unit shares with marginals.hip
#pragma once

#include <cstddef>

namespace gps {

// widest fat block served: Sigma_BB of a segment (its two fat blocks, 2 NB square, rounded up to the 16 columns of a tile) is staged
// once per workgroup in LDS by k_mg_fs_finish -- 128 x 130 doubles = 130 KB at NB = 64
constexpr int kMgFsMaxNB = 64;
// G = A_s^-1 H[I_s, B_s] overwrites the marginals' own copy of Y: row (state i, coordinate r) -> i b + r, NCP doubles each.  A wave of
// k_mg_fs_finish reads whole 16-row tiles of a 48-row group and the tile behind it: at most 63 rows past the last interior state's
constexpr int kMgFsPadRows = 64;
inline size_t mg_fs_grows(int N, int b) { return (size_t)N * b + kMgFsPadRows; }
inline int mg_fs_ldz(int NB) { return (2 * NB + 15) / 16 * 16; }

// gather modes of marginals_fs_gather (the three landmark getters)
enum { kMgGatherLmPair = 0, kMgGatherStateLm = 1 };

}  // namespace gps
