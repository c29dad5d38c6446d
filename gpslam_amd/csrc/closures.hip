// closures.hip -- the launches of the loop-closure kernels (closures.hpp; gpslam_hip_add_between_pairs).  Closures exist on fp64
// handles only (compile() refuses the others), so this is compiled once, like the marginals, and both precision namespaces of
// api_impl.inc call into it (api_common.hpp declares the entry points and says where each one stands in an iteration).
#include "api_common.hpp"
#include "marginals_dev.hpp"

namespace {

CloArgs clo_args(gpslam_hip_handle *h) {
  const Closures &c = h->clo;
  CloArgs a;
  a.pose = h->pose.as<double>(); a.stride = h->stride; a.count = c.n; a.chart = h->cfg.chart;
  a.first = c.fac.d_idx.as<int>(); a.second = c.d_second.as<int>();
  a.meas = c.fac.d_meas.as<double>(); a.sig = c.fac.d_sig.as<double>();
  a.A = c.A.as<double>(); a.partial = nullptr;
  a.rob = c.rob.empty() ? nullptr : c.d_rob.as<double>();
  a.blk = h->lv.empty() ? nullptr : h->lv[0].blk.as<double>();
  a.BS = 2 * h->b * h->b + h->b * h->R; a.B = h->b; a.R = h->R; a.col0 = 1 + h->nl;
  a.gsave = nullptr;
  a.x = h->lv.empty() ? nullptr : h->lv[0].x.as<double>();
  a.N = h->N; a.ncols = 1 + h->nl; a.Y = c.Y.as<double>(); a.flag = h->flag.as<int>();
  return a;
}
// closures in column passes: slice p of the compiled graph's closures, and what the pass kernels share
CloPass clo_pass(gpslam_hip_handle *h, int p) {
  const Closures &c = h->clo;
  CloPass cp;
  cp.k0 = std::min(p * c.slice, c.n); cp.k1 = std::min(cp.k0 + c.slice, c.n);
  cp.lead = p == 0 ? 1 : 0;
  cp.W = c.W.as<double>(); cp.ldw = clo_ldw(h); cp.X = c.X.as<double>();
  return cp;
}
// the leading columns (update + landmarks) of every state: what k_clo_save, k_clo_clear_lead and k_clo_add run over
int clo_nlead(const gpslam_hip_handle *h) { return h->N * (1 + h->nl) * h->b; }

}  // namespace

int closures_upload(gpslam_hip_handle *h) {
  Closures &c = h->clo;
  int rc;
  if ((rc = upload_set(h, c.fac, std::vector<int>()))) return rc;
  if ((rc = upload(h, c.d_second, c.second))) return rc;
  HIPCHK(c.A.reserve((size_t)c.n * kCloLen(h->d) * sizeof(double)));
  HIPCHK(c.Y.reserve((size_t)c.nc * (1 + h->nl) * sizeof(double)));
  if (c.P > 1) {
    HIPCHK(c.W.reserve((size_t)c.nc * clo_ldw(h) * sizeof(double)));
    HIPCHK(c.X.reserve((size_t)clo_nlead(h) * sizeof(double)));
    // (process-wide per kernel: always the size of the widest system)
    hipError_t ea = hipSuccess;
    dispatch_b(h->b, [&](auto tag) {
      ea = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_clo_solve_wide<decltype(tag)::value / 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCloWideLds);
    });
    HIPCHK(ea);
  }
  if ((rc = upload(h, c.d_rob, c.rob))) return rc;
  if (!c.rob.empty()) HIPCHK(c.w.reserve((size_t)c.n * sizeof(double)));
  return 0;
}

void closures_eval(gpslam_hip_handle *h, const LaunchMode &m, int pass, double *partial, hipStream_t st) {
  CloArgs a = clo_args(h);
  a.partial = partial;
  a.out_w = (m.weights && a.rob) ? h->clo.w.as<double>() : nullptr;
  dispatch_mf(h->mf, [&](auto tag) {
    constexpr int MF = decltype(tag)::value;
    if (pass == 0) k_clo_eval<MF, true><<<dim3(1), dim3(128), 0, st>>>(a);
    else k_clo_eval<MF, false><<<dim3(1), dim3(128), 0, st>>>(a);
  });
}

void closures_inject(gpslam_hip_handle *h, bool save_g, int pass) {
  CloArgs c = clo_args(h);
  c.gsave = save_g ? h->gsave.as<double>() : nullptr;
  if (h->clo.P > 1 && pass >= h->clo.P) {
    dispatch_b(h->b, [&](auto tag) {
      constexpr int D = decltype(tag)::value / 2;
      k_clo_clear_lead<D><<<dim3(nblocks(clo_nlead(h), 256)), dim3(256), 0, h->stream>>>(c);
      k_clo_inject_y<D><<<dim3(1), dim3(256), 0, h->stream>>>(c);
    });
  } else {
    const CloPass cp = clo_pass(h, pass);   // (one pass: every closure)
    dispatch_b(h->b, [&](auto tag) { k_clo_inject<decltype(tag)::value / 2><<<dim3(1), dim3(256), 0, h->stream>>>(c, cp.k0, cp.k1); });
  }
}

int closures_correct(gpslam_hip_handle *h) {
  if (h->clo.n <= 0) return 0;
  CloArgs a = clo_args(h);
  dispatch_b(h->b, [&](auto tag) {
    constexpr int D = decltype(tag)::value / 2;
    k_clo_solve<D><<<dim3(1), dim3(64), 0, h->stream>>>(a);
    k_clo_correct<D><<<dim3(nblocks(h->N * h->b, 256)), dim3(256), 0, h->stream>>>(a);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

void closures_collect(gpslam_hip_handle *h, int p, bool keep_z) {
  const CloArgs a = clo_args(h);
  const CloPass cp = clo_pass(h, p);
  const int wid = (cp.k1 - cp.k0) * h->d;
  const int entries = h->clo.nc * ((cp.lead ? a.ncols : 0) + wid);
  const size_t kept = (size_t)h->N * wid * h->b;
  dispatch_b(h->b, [&](auto tag) {
    constexpr int D = decltype(tag)::value / 2;
    if (keep_z) k_mg_keep_z<D><<<dim3((unsigned)((kept + 255) / 256)), dim3(256), 0, h->stream>>>(a, cp, h->mg.Z.as<double>(), mg_ldz(h->clo.nc));
    if (p == 0) k_clo_save<D><<<dim3(nblocks(clo_nlead(h), 256)), dim3(256), 0, h->stream>>>(a, cp);
    k_clo_gather<D><<<dim3(nblocks(entries, 256)), dim3(256), 0, h->stream>>>(a, cp);
    if (p == h->clo.P - 1) k_clo_solve_wide<D><<<dim3(1), dim3(256), clo_wide_lds(h->clo.nc, a.ncols), h->stream>>>(a, clo_pass(h, 0));
  });
}

int closures_add(gpslam_hip_handle *h) {
  const CloArgs a = clo_args(h);
  const CloPass cp = clo_pass(h, 0);
  dispatch_b(h->b, [&](auto tag) { k_clo_add<decltype(tag)::value / 2><<<dim3(nblocks(clo_nlead(h), 256)), dim3(256), 0, h->stream>>>(a, cp); });
  HIPCHK(hipGetLastError());
  return 0;
}
