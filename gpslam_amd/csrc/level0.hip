// level0.hip -- the one home of the level-0 forms that exist for fp64 solver records only (level0.hpp: k_chunk_forward_rows,
// k_fused_level0, k_chunk_backward_rows).  Every instantiation a handle can reach is named here, once, so this is the only unit that
// compiles them; the precision halves (api_impl.inc) call the launchers below through kernels.hpp's declarations.
#include "../../include/gpslam_hip.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "level0.hpp"

namespace gps {

namespace {
// (the census takes the instantiation from the text of the launch statement itself, at compile time: it cannot drift from it)
struct FusedId { int sv = 0, b = 12; bool fp32 = false, dg = false; };
constexpr FusedId fused_id(const char *s) {   // "k_fused_level0<SV[, TR[, B[, DG]]]>", the template's defaults where the text stops early
  FusedId id;
  while (*s != '<') ++s;
  id.sv = s[1] - '0';
  for (int field = 0; *s != '>'; ++s) {
    if (*s != ',') continue;
    while (s[1] == ' ') ++s;
    field++;
    if (field == 1) id.fp32 = s[1] == 'f';
    if (field == 2) { id.b = 0; for (const char *t = s + 1; *t >= '0' && *t <= '9'; ++t) id.b = id.b * 10 + (*t - '0'); }
    if (field == 3) id.dg = s[1] == 't';
  }
  return id;
}
static_assert(fused_id("k_fused_level0<4>").sv == 4 && fused_id("k_fused_level0<4>").b == 12 && !fused_id("k_fused_level0<4>").dg, "fused_id");
static_assert(fused_id("k_fused_level0<1,double,6>").sv == 1 && fused_id("k_fused_level0<1,double,6>").b == 6 && !fused_id("k_fused_level0<1,double,6>").fp32 &&
              fused_id("k_fused_level0<2,float,12,true>").dg && fused_id("k_fused_level0<2,float,12,true>").fp32 && fused_id("k_fused_level0<2,float,12,true>").b == 12, "fused_id");
static_assert(fused_id("k_fused_level0<3, double, 12, true>").dg && fused_id("k_fused_level0<0, float, 6>").fp32 && fused_id("k_fused_level0<0, float, 6>").b == 6, "fused_id");
// ea / eb != null: the launch carries its own start / stop events (a timed iteration: the dispatch's own time stamps)
// (expands inside launch_fused_k only: grid, st, ea, eb, u and the census array `cen` are that function's parameters)
#define GPS_FUSED_LAUNCH(...)                                                                                      \
  do {                                                                                                             \
    constexpr FusedId id_ = fused_id(#__VA_ARGS__);                                                                \
    cen[GPSLAM_CENSUS_L0_FUSED]++;                                                                                 \
    cen[GPSLAM_CENSUS_FUSED_SV] = id_.sv; cen[GPSLAM_CENSUS_FUSED_DG] = id_.dg; cen[GPSLAM_CENSUS_FUSED_B] = id_.b; \
    cen[GPSLAM_CENSUS_FUSED_FP32] = id_.fp32;                                                                      \
    if (ea) hipExtLaunchKernelGGL((__VA_ARGS__), dim3(grid), dim3(128), 0, st, ea, eb, 0, u);                      \
    else __VA_ARGS__<<<dim3(grid), dim3(128), 0, st>>>(u);                                                         \
  } while (0)
// the inputs of a k_fused_level0 launch as its arguments carry them (census)
template <typename TR> void census_fused_inputs(int32_t *cen, int b, const FusedArgs<double, TR> &u) {
  cen[GPSLAM_CENSUS_FUSED_GP] = u.gps == nullptr ? 0 : (b == 6 ? 1 : 2);
  cen[GPSLAM_CENSUS_FUSED_BTW_REC] = u.brec != nullptr;
  cen[GPSLAM_CENSUS_FUSED_LINES] = u.rowI != nullptr;
  cen[GPSLAM_CENSUS_FUSED_ODD_ROWS] = u.odd_rows;
  cen[GPSLAM_CENSUS_FUSED_GSAVE] = u.gsave != nullptr;
  cen[GPSLAM_CENSUS_FUSED_TAIL] = u.f.tail != 0;
  cen[GPSLAM_CENSUS_FUSED_GSAVE_LAUNCHES] += u.gsave != nullptr;
  cen[GPSLAM_CENSUS_FUSED_TAIL_LAUNCHES] += u.f.tail != 0;
}
}  // namespace

void launch_fused_k(int32_t *cen, int b, int sv, bool dg, const FusedArgs<double, double> &u, int grid, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
  census_fused_inputs(cen, b, u);
  if (b == 6) {
    if (sv == 1) GPS_FUSED_LAUNCH(k_fused_level0<1, double, 6>);      // d = 3 records (kGp3*)
    else GPS_FUSED_LAUNCH(k_fused_level0<0, double, 6>);
    return;
  }
  switch (sv) {
    case 4:                                  // records + interpolated measurement rows as 16-double lines (round 5)
      if (dg) GPS_FUSED_LAUNCH(k_fused_level0<4, double, 12, true>);
      else GPS_FUSED_LAUNCH(k_fused_level0<4>);
      break;
    case 3:                                  // records + a ring of full-width rows (measurement factors)
      if (dg) GPS_FUSED_LAUNCH(k_fused_level0<3, double, 12, true>);
      else GPS_FUSED_LAUNCH(k_fused_level0<3>);
      break;
    case 2: GPS_FUSED_LAUNCH(k_fused_level0<2>); break;
    case 1:
      if (dg) GPS_FUSED_LAUNCH(k_fused_level0<1, double, 12, true>);   // diagonal chol(Qc^-1)
      else GPS_FUSED_LAUNCH(k_fused_level0<1>);
      break;
    default: GPS_FUSED_LAUNCH(k_fused_level0<0>);
  }
}
// fp32 handles: fp32 row tables straight into the fused kernel's fp64 accumulation (round 3: the unfused assembly had cost the
// fp32 mode more than its halved row traffic saved)
void launch_fused_k(int32_t *cen, int b, int, bool, const FusedArgs<double, float> &u, int grid, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
  census_fused_inputs(cen, b, u);
  if (b == 6) GPS_FUSED_LAUNCH(k_fused_level0<0, float, 6>);
  else GPS_FUSED_LAUNCH(k_fused_level0<0, float>);
}
void launch_rows_k(int32_t *cen, int b, const FwdArgs<double> &a, int grid, hipStream_t st) {
  cen[GPSLAM_CENSUS_L0_ROWS]++;
  if (b == 12) k_chunk_forward_rows<12><<<dim3(grid), dim3(64), 0, st>>>(a);
  else if (b == 6) k_chunk_forward_rows<6><<<dim3(grid), dim3(64), 0, st>>>(a);
  else k_chunk_forward_rows<4><<<dim3(grid), dim3(64), 0, st>>>(a);
}
void launch_bwd_rows_k(int32_t *cen, int b, const BwdArgs<double> &a, int grid, hipStream_t st) {
  cen[GPSLAM_CENSUS_BWD_ROWS]++;
  cen[GPSLAM_CENSUS_BWD_ROWS_FOLD] += a.l1_blk != nullptr;
  if (b == 12) k_chunk_backward_rows<12><<<dim3(grid), dim3(64), 0, st>>>(a);
  else if (b == 6) k_chunk_backward_rows<6><<<dim3(grid), dim3(64), 0, st>>>(a);
  else k_chunk_backward_rows<4><<<dim3(grid), dim3(64), 0, st>>>(a);
}

}  // namespace gps
