// The SE(2) / SO(3) factors of gpslam_amd/csrc/factors.hpp in hipcc's HOST pass against the 50-digit branch pins
// (tests/golden/d3_branch_pins.json): the functions are __host__ __device__, so a wrong branch or sign shows here, on the CPU.
//   GpPrior<double, POSE2 / ROT3, true>::eval, interp_pose2 / interp_rot3<double, true>, PoseFactors<double, POSE2 / ROT3, true>::prior / between
// Input: the text file tests/test_d3_branch_host.py writes from the pins, one case per line
//   kind what chart  n_in in...  n_out pin... tol...
// kind 2 = POSE2, 4 = ROT3; what 0 = GP prior (p1 v1 p2 v2 dt), 1 = interpolation (p1 v1 p2 v2 dt tau), 2 = prior (m x), 3 = between (m x1 x2).
// Every output entry must lie within its tol of its pin (8 noise + 8 u |exact|; an entry whose tol is zero is met exactly).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../gpslam_amd/csrc/factors.hpp"

using namespace gps;

// First block row of Lambda(tau), Psi(tau).  A COPY of the library's host-side interp_coef (api_common.hpp, which this program cannot
// include without the whole handle), not a call to it: a wrong coefficient in the library does not show here, only in
// tests/test_gpu_d3_branch_pins.py (interpolate_poses_jac).  Qc cancels in Lambda and Psi, so the pins' non-diagonal Qc reaches
// neither this program nor the kernel: it is in the generator's Lambda / Psi and the oracle's, which is where it could go wrong.
static ICoef<double> icoef(double dt, double tau) {
  const double s = dt - tau;
  const double a11 = tau * tau * tau / 3.0 + s * tau * tau / 2.0, a12 = tau * tau / 2.0;
  const double p11 = a11 * (12.0 / (dt * dt * dt)) + a12 * (-6.0 / (dt * dt));
  const double p12 = a11 * (-6.0 / (dt * dt)) + a12 * (4.0 / dt);
  return {1.0 - p11, tau - p11 * dt - p12, p11, p12};
}

template <int MF> static void run_gp(const double *in, std::vector<double> &out) {
  constexpr int pd = MTraits<MF>::pd;
  double e[6], Jt[36], Jb[36];
  GpPrior<double, MF, true>::eval(in, in + pd, in + pd + 3, in + 2 * pd + 3, in[2 * pd + 6], e, Jt, Jb);
  out.assign(e, e + 6);
  for (int m = 0; m < 4; m++)
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 3; c++) out.push_back(r < 3 ? Jt[r * 12 + 3 * m + c] : Jb[(r - 3) * 12 + 3 * m + c]);
}

static void push(std::vector<double> &out, const M3<double> &a) { out.insert(out.end(), a.m, a.m + 9); }

template <int MF> static void run_interp(const double *in, std::vector<double> &out) {
  constexpr int pd = MTraits<MF>::pd;
  const ICoef<double> k = icoef(in[2 * pd + 6], in[2 * pd + 7]);
  Interp3Out<double, true> o;
  out.clear();
  if (MF == POSE2) {
    const SE2<double> p = interp_pose2<double, true>(in, in + pd, in + pd + 3, in + 2 * pd + 3, k, o);
    out = {p.x, p.y, p.th};
  } else {
    push(out, interp_rot3<double, true>(in, in + pd, in + pd + 3, in + 2 * pd + 3, k, o));
  }
  push(out, o.H1); push(out, o.H2); push(out, o.H3); push(out, o.H4);
}

template <int MF> static void run_prior(const double *in, int chart, std::vector<double> &out) {
  constexpr int pd = MTraits<MF>::pd;
  double e[3], H[9];
  PoseFactors<double, MF, true>::prior(in, in + pd, chart, e, H);
  out.assign(e, e + 3);
  out.insert(out.end(), H, H + 9);
}

template <int MF> static void run_between(const double *in, int chart, std::vector<double> &out) {
  constexpr int pd = MTraits<MF>::pd;
  double e[3], H1[9], H2[9];
  PoseFactors<double, MF, true>::between(in, in + pd, in + 2 * pd, chart, e, H1, H2);
  out.assign(e, e + 3);
  out.insert(out.end(), H1, H1 + 9);
  out.insert(out.end(), H2, H2 + 9);
}

int main(int argc, char **argv) {
  if (argc != 2) { std::printf("usage: %s cases.txt\n", argv[0]); return 2; }
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int kind, what, chart, n_in, n_out, cases = 0, fails = 0;
  double worst[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  while (std::fscanf(f, "%d %d %d %d", &kind, &what, &chart, &n_in) == 4) {
    std::vector<double> in(n_in), out;
    for (double &x : in) if (std::fscanf(f, "%lf", &x) != 1) return 2;
    if (std::fscanf(f, "%d", &n_out) != 1) return 2;
    std::vector<double> pin(n_out), tol(n_out);
    for (double &x : pin) if (std::fscanf(f, "%lf", &x) != 1) return 2;
    for (double &x : tol) if (std::fscanf(f, "%lf", &x) != 1) return 2;
    const bool p2 = kind == POSE2;
    if (!p2 && kind != ROT3) return 2;
    if (what == 0) p2 ? run_gp<POSE2>(in.data(), out) : run_gp<ROT3>(in.data(), out);
    else if (what == 1) p2 ? run_interp<POSE2>(in.data(), out) : run_interp<ROT3>(in.data(), out);
    else if (what == 2) p2 ? run_prior<POSE2>(in.data(), chart, out) : run_prior<ROT3>(in.data(), chart, out);
    else if (what == 3) p2 ? run_between<POSE2>(in.data(), chart, out) : run_between<ROT3>(in.data(), chart, out);
    else return 2;
    if ((int)out.size() != n_out) { std::printf("FAIL case %d: %d outputs, %d pins\n", cases, (int)out.size(), n_out); return 1; }
    for (int i = 0; i < n_out; i++) {
      const double d = std::fabs(out[i] - pin[i]);
      const bool ok = tol[i] > 0.0 ? d <= tol[i] : d == 0.0;        // (a NaN fails either)
      if (tol[i] > 0.0 && d == d) worst[p2 ? 0 : 1][what] = std::fmax(worst[p2 ? 0 : 1][what], d / tol[i]);
      if (!ok) {
        fails++;
        std::printf("FAIL case %d (kind %d what %d chart %d) entry %d: got %.17g pin %.17g tol %.3g\n", cases, kind, what, chart, i, out[i], pin[i], tol[i]);
      }
    }
    cases++;
  }
  std::fclose(f);
  const char *names[4] = {"gp_prior", "interp", "prior", "between"};
  for (int k = 0; k < 2; k++)
    for (int w = 0; w < 4; w++) std::printf("%s %s: worst host pass / tol %.3g\n", k ? "rot3" : "pose2", names[w], worst[k][w]);
  if (fails || !cases) { std::printf("%d entries out of tolerance in %d cases\n", fails, cases); return 1; }
  std::printf("all d3 branch host tests passed (%d cases)\n", cases);
  return 0;
}
