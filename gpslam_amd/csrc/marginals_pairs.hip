// marginals_pairs.hip -- Sigma_{a,b} of ANY two states (gpslam_hip_get_state_pair_marginals) and the chi-square gate of loop-closure
// candidates over it (gpslam_hip_gate_between_pairs), from what gpslam_hip_marginals leaves on the device.  A translation unit of
// its own: the kernels of marginals.hip, marginals_clo.hip and closures.hip stay what they were, byte for byte.
//
//   Sigma_xx = A^-1 + (low-rank term), A the block-tridiagonal chain part, so Sigma_{a,b} = A^-1_{a,b} + the same term between rows a, b.
//
//   (a) A^-1_{a,b} through the hierarchy of the selected inversion (k_mg_pair, one wave per pair).  The records [P_j^-1 | U_j | V_j] of
//       mg.fac (level 0) and mg.up (the levels above), with x_j = P_j^-1 r_j - U_j x_{j+1} - V_j x_s, are a block L D L^T of A in the
//       elimination order, and Sigma_top (the top level's one block) closes it.  Hence
//           A^-1_{a,b} = (L^-1 E_a)^T D^-1 (L^-1 E_b) = sum_i (r^a_i)^T P_i^-1 r^b_i + (r^a_top)^T Sigma_top r^b_top,
//       r^a, r^b the forward sweeps of the identity block at a and at b:  r_{j+1} -= U_j^T r_j,  r_s -= V_j^T r_j  (the last interior's
//       U_j^T r_j goes to the right separator; the separators' blocks are the next level's right-hand side).  At every level a sweep is
//       non-zero on at most two adjacent items (p, p + 1) and touches only the interiors from there to the end of p's chunk; the two
//       sweeps meet only in a chunk they share.  Both sweeps run in one loop: no backward walk, nothing stored per level, 6 block
//       products per interior both sides visit and 2 per interior one side visits -- at most about 6 * 15 per level, whatever |a - b|.
//       Every address follows from the indices, so the next interior's record is requested into registers before the current one's
//       arithmetic starts (as k_head_schur does).
//   (b) the low-rank term and the output rules (k_mg_pair_finish, a thread per pair and row): single pass + Y_a K Y_b^T with mg.K;
//       column passes + W_a S^-1 W_b^T - Z_a M^-1 Z_b^T with mg.K (= S^-1 there), mg.Z, mg.Minv.  Y = [W | Z] is read from mg.Y, the
//       copy gpslam_hip_marginals makes under gpslam_hip_marginals_keep_pair_terms (k_mg_keep_y): the solver's own buffer is rewritten
//       by later calls.  a == b and |a - b| == 1 are copies of mg.S / mg.Sn; every other pair is computed for (min, max) by one code
//       path and transposed on output.
//   (c) the gate (k_mg_gate, a thread per candidate): e, H1, H2 of BetweenFactor at the current states (PoseFactors::between, as
//       k_clo_eval), P = diag(sigma^2) + [H1 H2] Sigma^{pp} [H1 H2]^T from the three pair blocks, chi2 = e^T P^-1 e by Cholesky.
// fp64 only; no atomics, every sum in a fixed order: two calls give bit-identical blocks.  tests/marginals_pairs_model.py is (a), (b) in numpy.
// The levels are read through marginals.hpp's MgLevels, the one description of what gpslam_hip_marginals laid out; mg_set is marginals_dev.hpp's.
#include "marginals_dev.hpp"

namespace {

struct MgPair {
  const double *fac[kMgMaxLevels];   // per level below the top: n[l] x 3 B^2 records [P^-1 | U | V]
  int n[kMgMaxLevels];
  int top;                           // levels 0 .. top - 1 are swept; level top is one block
  const double *Stop;                // Sigma of the top block
  const int *a, *b;                  // the pairs as asked for (either order)
  int count;
  double *out;                       // count x B^2: A^-1_{min, max} (rows: min); untouched where |a - b| < 2
};

template <int B> __global__ void __launch_bounds__(64) k_mg_pair(MgPair a) {
  constexpr int BB = B * B, NE = (BB + 63) / 64;
  __shared__ double Cur[2][BB], Sep[2][BB], R0[2][BB], R1[2][BB], Pi[BB], U[BB], V[BB], T[BB], Acc[BB];
  const int t = blockIdx.x;
  int p[2] = {min(a.a[t], a.b[t]), max(a.a[t], a.b[t])};
  if (p[1] - p[0] < 2) return;
  bool has1[2] = {false, false};
  for (int s = 0; s < 2; s++) {
    mg_set<B>(R0[s], [&](int r, int c) { return r == c ? 1.0 : 0.0; });
    mg_set<B>(R1[s], [&](int, int) { return 0.0; });
  }
  mg_set<B>(Acc, [&](int, int) { return 0.0; });
  double pre[3][NE];
  auto request = [&](const double *f) {
#pragma unroll
    for (int u = 0; u < NE; u++) {
      const int e = threadIdx.x + 64 * u;
      if (e < BB) { pre[0][u] = f[e]; pre[1][u] = f[BB + e]; pre[2][u] = f[2 * BB + e]; }
    }
  };
  for (int l = 0; l < a.top; l++) {
    const int n = a.n[l];
    const double *fac = a.fac[l];
    int c[2], e[2], start[2];
    bool nz[2] = {false, false};      // Cur[s] holds a right-hand side (behind the loop: what the last interior hands to the right)
    for (int s = 0; s < 2; s++) {
      c[s] = p[s] / kMgChunk;
      e[s] = min(c[s] * kMgChunk + kMgChunk, n);
      start[s] = (p[s] == c[s] * kMgChunk && !has1[s]) ? e[s] : max(p[s], c[s] * kMgChunk + 1);   // a lone separator sweeps nothing
      mg_set<B>(Sep[s], [&](int, int) { return 0.0; });
    }
    const bool same = c[0] == c[1];
    for (int g = 0; g < (same ? 1 : 2); g++) {
      const int s0 = same ? 0 : g, s1 = same ? 1 : g;
      const int jbeg = min(start[s0], start[s1]), jend = e[s0];
      if (jbeg < jend) request(fac + (size_t)jbeg * 3 * BB);
      for (int j = jbeg; j < jend; j++) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NE; u++) {
          const int q = threadIdx.x + 64 * u;
          if (q < BB) { Pi[q] = pre[0][u]; U[q] = pre[1][u]; V[q] = pre[2][u]; }
        }
        __syncthreads();
        if (j + 1 < jend) request(fac + (size_t)(j + 1) * 3 * BB);
        for (int s = s0; s <= s1; s++) {
          if (j < start[s]) continue;
          const double *add = (j == p[s]) ? R0[s] : (has1[s] && j == p[s] + 1) ? R1[s] : nullptr;
          if (!add) continue;
          const bool had = nz[s];
          mg_set<B>(Cur[s], [&](int r, int cc) { return (had ? Cur[s][r * B + cc] : 0.0) + add[r * B + cc]; });
          nz[s] = true;
        }
        if (same && nz[0] && nz[1]) {
          mg_set<B>(T, [&](int r, int cc) { double acc = 0.0; for (int q = 0; q < B; q++) acc += Pi[r * B + q] * Cur[1][q * B + cc]; return acc; });
          mg_set<B>(Acc, [&](int r, int cc) { double acc = Acc[r * B + cc]; for (int q = 0; q < B; q++) acc += Cur[0][q * B + r] * T[q * B + cc]; return acc; });
        }
        for (int s = s0; s <= s1; s++) {
          if (!nz[s]) continue;
          mg_set<B>(Sep[s], [&](int r, int cc) { double acc = Sep[s][r * B + cc]; for (int q = 0; q < B; q++) acc -= V[q * B + r] * Cur[s][q * B + cc]; return acc; });
          mg_set<B>(Cur[s], [&](int r, int cc) { double acc = 0.0; for (int q = 0; q < B; q++) acc -= U[q * B + r] * Cur[s][q * B + cc]; return acc; });
        }
      }
    }
    for (int s = 0; s < 2; s++) {     // the next level's right-hand side: items c[s] (this chunk's separator) and c[s] + 1 (the right one)
      const bool own = p[s] == c[s] * kMgChunk, right = e[s] < n;
      const bool carry = right && nz[s], sepr = right && has1[s] && p[s] + 1 == e[s];
      mg_set<B>(R0[s], [&](int r, int cc) { return Sep[s][r * B + cc] + (own ? R0[s][r * B + cc] : 0.0); });
      mg_set<B>(R1[s], [&](int r, int cc) { return (carry ? Cur[s][r * B + cc] : 0.0) + (sepr ? R1[s][r * B + cc] : 0.0); });
      p[s] = c[s];
      has1[s] = right;
    }
  }
  mg_set<B>(Pi, [&](int r, int cc) { return a.Stop[r * B + cc]; });
  mg_set<B>(T, [&](int r, int cc) { double acc = 0.0; for (int q = 0; q < B; q++) acc += Pi[r * B + q] * R0[1][q * B + cc]; return acc; });
  mg_set<B>(Acc, [&](int r, int cc) { double acc = Acc[r * B + cc]; for (int q = 0; q < B; q++) acc += R0[0][q * B + r] * T[q * B + cc]; return acc; });
  for (int q = threadIdx.x; q < BB; q += 64) a.out[(size_t)t * BB + q] = Acc[q];
}

// mg.Y[(i m + q) B + k] = x[(i R + 1 + q) B + k], q < m: the columns behind the update column of every state's level-0 solution
__global__ void __launch_bounds__(256) k_mg_keep_y(const double *x, double *Y, int N, int R, int m, int B) {
  const int per = m * B;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)N * per) return;
  const size_t s = i / per;
  Y[i] = x[(s * R + 1) * B + (i - s * per)];
}

struct MgPairFinish {
  const double *chain;          // k_mg_pair's blocks
  const int *a, *b;
  int count, N;
  const double *Sd, *Sn;        // mg.S, mg.Sn
  const double *Y, *K;          // mg.Y (N x m x B), mg.K (m x m)
  int m;
  const double *Z, *Minv;       // column passes: mg.Z, mg.Minv, or null
  int nc, ldz;
  int pad0, npad;
  double *out;                  // count x B^2: Sigma_{a[t], b[t]}
};
template <int B> __global__ void __launch_bounds__(256) k_mg_pair_finish(MgPairFinish a) {
  constexpr int BB = B * B;
  const int tid = blockIdx.x * 256 + threadIdx.x;
  const int t = tid / B, r = tid - t * B;
  if (t >= a.count) return;
  const int ia = a.a[t], ib = a.b[t], lo = min(ia, ib), hi = max(ia, ib);
  double *out = a.out + (size_t)t * BB;
  if (lo == hi) {
    for (int c = 0; c < B; c++) out[r * B + c] = a.Sd[(size_t)lo * BB + r * B + c];
    return;
  }
  if (hi == lo + 1) {
    for (int c = 0; c < B; c++) out[r * B + c] = ia < ib ? a.Sn[(size_t)lo * BB + r * B + c] : a.Sn[(size_t)lo * BB + c * B + r];
    return;
  }
  // row r of Sigma_{lo,hi}, one code path for both orders
  double acc[B];
#pragma unroll
  for (int c = 0; c < B; c++) acc[c] = a.chain[(size_t)t * BB + r * B + c];
  if (a.m > 0) {
    const double *yl = a.Y + (size_t)lo * a.m * B, *yh = a.Y + (size_t)hi * a.m * B;
    for (int q2 = 0; q2 < a.m; q2++) {
      double tq = 0.0;
      for (int q = 0; q < a.m; q++) tq += yl[q * B + r] * a.K[q * a.m + q2];
#pragma unroll
      for (int c = 0; c < B; c++) acc[c] += tq * yh[q2 * B + c];
    }
  }
  if (a.Z) {
    const double *zl = a.Z + ((size_t)lo * B + r) * a.ldz, *zh = a.Z + (size_t)hi * B * a.ldz;
    for (int q2 = 0; q2 < a.nc; q2++) {
      double tq = 0.0;
      for (int q = 0; q < a.nc; q++) tq += zl[q] * a.Minv[(size_t)q * a.ldz + q2];
#pragma unroll
      for (int c = 0; c < B; c++) acc[c] -= tq * zh[(size_t)c * a.ldz + q2];
    }
  }
  const bool rp = a.npad > 0 && r >= a.pad0 && r < a.pad0 + a.npad;
#pragma unroll
  for (int c = 0; c < B; c++) {
    const bool cp = a.npad > 0 && c >= a.pad0 && c < a.pad0 + a.npad;
    const double v = (rp || cp) ? 0.0 : acc[c];
    if (ia < ib) out[r * B + c] = v;
    else out[c * B + r] = v;
  }
}

struct MgGate {
  const double *pose;
  int stride, count, chart, B;
  const int *first, *second;
  const double *meas, *sig;     // count x pd, count x d
  const double *S;              // 3 count x B^2: Sigma_{f,f}, Sigma_{f,s}, Sigma_{s,s} of candidate t at blocks 3 t .. 3 t + 2
  double *err, *P, *chi2;       // count x d, count x d x d, count
  int *flag;
};
template <int MF> __global__ void __launch_bounds__(64) k_mg_gate(MgGate a) {
  constexpr int d = MTraits<MF>::d, pd = MTraits<MF>::pd;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.count) return;
  const int i = a.first[f], j = a.second[f], B = a.B;
  double x1[pd], x2[pd], m[pd], e[d], H1[d * d], H2[d * d];
#pragma unroll
  for (int k = 0; k < pd; k++) {
    x1[k] = a.pose[(size_t)k * a.stride + i];
    x2[k] = a.pose[(size_t)k * a.stride + j];
    m[k] = a.meas[(size_t)f * pd + k];
  }
  PoseFactors<double, MF, true>::between(m, x1, x2, a.chart, e, H1, H2);
  const double *Sff = a.S + (size_t)(3 * f) * B * B, *Sfs = Sff + B * B, *Sss = Sfs + B * B;
  // G(X, S, Y)[r][c] = sum_u sum_v X[r][u] S[u][v] Y[c][v] over the pose-tangent block (the leading d x d entries of a b x b block)
  auto quad = [&](const double *X, const double *S, const double *Y, int r, int c) {
    double acc = 0.0;
    for (int u = 0; u < d; u++) {
      double tv = 0.0;
      for (int v = 0; v < d; v++) tv += S[u * B + v] * Y[c * d + v];
      acc += X[r * d + u] * tv;
    }
    return acc;
  };
  double C[d * d], P[d * d];
  for (int r = 0; r < d; r++)
    for (int c = 0; c < d; c++) C[r * d + c] = quad(H1, Sfs, H2, r, c);
  for (int r = 0; r < d; r++)
    for (int c = 0; c <= r; c++) {
      const double sg = a.sig[(size_t)f * d + r];
      const double v = (r == c ? sg * sg : 0.0) + quad(H1, Sff, H1, r, c) + (C[r * d + c] + C[c * d + r]) + quad(H2, Sss, H2, r, c);
      P[r * d + c] = v;
      P[c * d + r] = v;
    }
  if (a.err)
    for (int r = 0; r < d; r++) a.err[(size_t)f * d + r] = e[r];
  if (a.P)
    for (int r = 0; r < d * d; r++) a.P[(size_t)f * d * d + r] = P[r];
  // P = L L^T (lower triangle in place), y = L^-1 e, chi2 = |y|^2
  double chi = 0.0;
  for (int jj = 0; jj < d; jj++) {
    double dd = P[jj * d + jj];
    for (int k = 0; k < jj; k++) dd -= P[jj * d + k] * P[jj * d + k];
    if (!(dd > 0.0)) { *a.flag = 1; dd = 1.0; }      // (every writer writes the same value)
    const double l = sqrt(dd);
    P[jj * d + jj] = l;
    for (int r = jj + 1; r < d; r++) {
      double v = P[r * d + jj];
      for (int k = 0; k < jj; k++) v -= P[r * d + k] * P[jj * d + k];
      P[r * d + jj] = v / l;
    }
    double y = e[jj];
    for (int k = 0; k < jj; k++) y -= P[jj * d + k] * e[k];
    y /= l;
    e[jj] = y;
    chi += y * y;
  }
  a.chi2[f] = chi;
}

struct PairScratch { DevBuf a, b, chain, out, meas, sig, err, P, chi2; };   // one getter call's own buffers

int pairs_check(gpslam_hip_handle *h, const char *who) {
  int rc = marginals_getter_check(h);
  if (rc) return rc;
  if (h->fs.active) {
    h->err = std::string(who) + ": pairs of states on the segmented landmark path are not supported (the fat chain is not walked for a pair)";
    return GPSLAM_E_UNSUPPORTED;
  }
  if (!h->mg.pairs_ok) {
    h->err = std::string(who) + ": the handle has landmarks or closures and the last gpslam_hip_marginals() kept no copy of their columns: call "
             "gpslam_hip_marginals_keep_pair_terms(h, 1), then gpslam_hip_marginals() again";
    return GPSLAM_E_INVALID;
  }
  return 0;
}

// Sigma_{a[t], b[t]} into sc.out (device), the indices already checked; sc.a / sc.b stay uploaded
int pairs_on_device(gpslam_hip_handle *h, PairScratch &sc, const std::vector<int> &a, const std::vector<int> &b) {
  const int count = (int)a.size(), N = h->N, B = h->b, BB = B * B;
  int rc;
  if ((rc = upload(h, sc.a, a)) || (rc = upload(h, sc.b, b))) return rc;
  HIPCHK(sc.chain.reserve((size_t)count * BB * sizeof(double)));
  HIPCHK(sc.out.reserve((size_t)count * BB * sizeof(double)));
  bool far = false;
  for (int t = 0; t < count && !far; t++) far = std::abs(a[t] - b[t]) > 1;
  if (far) {
    MgPair p;
    const MgLevels lv(N, B);    // (as gpslam_hip_marginals laid them out)
    const int top = lv.top;
    const double *up = h->mg.up.as<double>();
    for (int l = 0; l < kMgMaxLevels; l++) {
      p.fac[l] = l >= top ? nullptr : l == 0 ? h->mg.fac.as<double>() : up + lv.fac(l);
      p.n[l] = l < top ? lv.n[l] : 0;
    }
    p.Stop = top == 0 ? h->mg.S.as<double>() : up + lv.Sd(top);
    p.top = top; p.a = sc.a.as<int>(); p.b = sc.b.as<int>(); p.count = count; p.out = sc.chain.as<double>();
    dispatch_b(B, [&](auto tag) { k_mg_pair<decltype(tag)::value><<<dim3(count), dim3(64), 0, h->stream>>>(p); });
  }
  const bool passes = h->clo.P > 1;
  MgPairFinish f;
  f.chain = sc.chain.as<double>(); f.a = sc.a.as<int>(); f.b = sc.b.as<int>(); f.count = count; f.N = N;
  f.Sd = h->mg.S.as<double>(); f.Sn = h->mg.Sn.as<double>();
  f.Y = h->mg.Y.as<double>(); f.K = h->mg.K.as<double>(); f.m = h->mg.Ym;
  f.Z = passes ? h->mg.Z.as<double>() : nullptr; f.Minv = passes ? h->mg.Minv.as<double>() : nullptr;
  f.nc = passes ? h->clo.nc : 0; f.ldz = passes ? mg_ldz(h->clo.nc) : 0;
  f.pad0 = mg_pads(h).pad0; f.npad = mg_pads(h).npad;
  f.out = sc.out.as<double>();
  dispatch_b(B, [&](auto tag) { k_mg_pair_finish<decltype(tag)::value><<<dim3(nblocks(count * B, 256)), dim3(256), 0, h->stream>>>(f); });
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

int marginals_pairs_keep(gpslam_hip_handle *h) {
  const int m = h->R - 1;
  h->mg.Ym = 0;
  if (m == 0) { h->mg.pairs_ok = true; return 0; }     // no landmarks, no closures: nothing to copy
  if (!h->mg.keep_pairs) return 0;
  const int my = h->clo.P > 1 ? h->nl : m;             // column passes: W alone, Z is in mg.Z
  if (my > 0) {
    HIPCHK(h->mg.Y.reserve((size_t)h->N * my * h->b * sizeof(double)));
    const size_t total = (size_t)h->N * my * h->b;
    k_mg_keep_y<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream>>>(h->lv[0].x.as<double>(), h->mg.Y.as<double>(), h->N, h->R, my, h->b);
    HIPCHK(hipGetLastError());
  }
  h->mg.Ym = my;
  h->mg.pairs_ok = true;
  return 0;
}

extern "C" {

int gpslam_hip_marginals_keep_pair_terms(gpslam_hip_handle *h, int32_t enable) {
  if (!h) return GPSLAM_E_INVALID;
  h->mg.invalidate();
  h->mg.keep_pairs = enable != 0;
  if (!h->mg.keep_pairs) h->mg.Y.release();   // freed now: N x m x b doubles that nothing reads without the opt-in
  return 0;
}

int gpslam_hip_get_state_pair_marginals(gpslam_hip_handle *h, int32_t count, const int32_t *a, const int32_t *b, double *out) {
  if (!h || count < 0 || (count > 0 && (!a || !b || !out))) return GPSLAM_E_INVALID;
  int rc = pairs_check(h, "get_state_pair_marginals");
  if (rc) return rc;
  for (int t = 0; t < count; t++)
    if (a[t] < 0 || a[t] >= h->N || b[t] < 0 || b[t] >= h->N) {
      h->err = "get_state_pair_marginals: item " + std::to_string(t) + ": state index out of range";
      return GPSLAM_E_INVALID;
    }
  if (count == 0) return 0;
  (void)hipSetDevice(h->cfg.device);
  PairScratch sc;
  if ((rc = pairs_on_device(h, sc, std::vector<int>(a, a + count), std::vector<int>(b, b + count)))) return rc;
  HIPCHK(hipMemcpyAsync(out, sc.out.p, (size_t)count * h->b * h->b * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int gpslam_hip_gate_between_pairs(gpslam_hip_handle *h, int32_t count, const int32_t *first, const int32_t *second,
                                  const double *measured, const double *sigmas, double *chi2, double *err, double *innov_cov) {
  if (!h || count < 0 || (count > 0 && (!first || !second || !measured || !sigmas || !chi2))) return GPSLAM_E_INVALID;
  int rc = pairs_check(h, "gate_between_pairs");
  if (rc) return rc;
  const int d = h->d, pd = h->pd;
  for (int t = 0; t < count; t++) {
    if (first[t] < 0 || first[t] >= h->N || second[t] < 0 || second[t] >= h->N) {
      h->err = "gate_between_pairs: item " + std::to_string(t) + ": state index out of range";
      return GPSLAM_E_INVALID;
    }
    if (first[t] == second[t]) {
      h->err = "gate_between_pairs: item " + std::to_string(t) + ": a BetweenFactor needs two different states";
      return GPSLAM_E_INVALID;
    }
  }
  for (size_t k = 0; k < (size_t)count * d; k++)
    if (!(sigmas[k] > 0.0)) return fail(h, GPSLAM_E_INVALID, "gate_between_pairs: sigmas must be positive");
  if (count == 0) return 0;
  (void)hipSetDevice(h->cfg.device);
  std::vector<int> pa((size_t)3 * count), pb((size_t)3 * count), fi(first, first + count), se(second, second + count);
  for (int t = 0; t < count; t++) {
    pa[3 * (size_t)t] = first[t]; pb[3 * (size_t)t] = first[t];
    pa[3 * (size_t)t + 1] = first[t]; pb[3 * (size_t)t + 1] = second[t];
    pa[3 * (size_t)t + 2] = second[t]; pb[3 * (size_t)t + 2] = second[t];
  }
  PairScratch sc;
  if ((rc = pairs_on_device(h, sc, pa, pb))) return rc;
  if ((rc = upload(h, sc.a, fi)) || (rc = upload(h, sc.b, se))) return rc;   // (upload drains the stream: the pair kernels are done with the lists)
  if ((rc = upload(h, sc.meas, std::vector<double>(measured, measured + (size_t)count * pd)))) return rc;
  if ((rc = upload(h, sc.sig, std::vector<double>(sigmas, sigmas + (size_t)count * d)))) return rc;
  HIPCHK(sc.err.reserve((size_t)count * d * sizeof(double)));
  HIPCHK(sc.P.reserve((size_t)count * d * d * sizeof(double)));
  HIPCHK(sc.chi2.reserve((size_t)count * sizeof(double)));
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  MgGate g;
  g.pose = h->pose.as<double>(); g.stride = h->stride; g.count = count; g.chart = h->cfg.chart; g.B = h->b;
  g.first = sc.a.as<int>(); g.second = sc.b.as<int>(); g.meas = sc.meas.as<double>(); g.sig = sc.sig.as<double>();
  g.S = sc.out.as<double>(); g.err = sc.err.as<double>(); g.P = sc.P.as<double>(); g.chi2 = sc.chi2.as<double>();
  g.flag = h->flag.as<int>();
  dispatch_mf(h->mf, [&](auto tag) { k_mg_gate<decltype(tag)::value><<<dim3(nblocks(count, 64)), dim3(64), 0, h->stream>>>(g); });
  HIPCHK(hipGetLastError());
  int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(chi2, sc.chi2.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (err) HIPCHK(hipMemcpyAsync(err, sc.err.p, (size_t)count * d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (innov_cov) HIPCHK(hipMemcpyAsync(innov_cov, sc.P.p, (size_t)count * d * d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (flag) return fail(h, GPSLAM_E_NOT_SPD, "gate_between_pairs: non-positive pivot in the innovation covariance");
  return 0;
}

}  // extern "C"
