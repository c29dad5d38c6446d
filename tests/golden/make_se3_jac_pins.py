#!/usr/bin/env python3
"""50-digit pins of the SE(3) GP factors' Jacobians, small relative rotations included: tests/golden/se3_jac_pins.json
and, for `H_exact`, tests/golden/se3_jac_pins_exact.json.

The reference's formulas (restated once in tests/se3_bounds.py, generic in the number type) are evaluated in mpmath at
50 digits, with the reference's branches and constants:
  * GaussianProcessPriorPose3::evaluateError H1..H4      gpslam/gp/GaussianProcessPriorPose3.h:60-98
  * GaussianProcessInterpolatorPose3::interpolatePose H1..H4, non-diagonal Qc, tau in {0.3, 1, -0.1, 1.1} dt
                                                          gpslam/gp/GaussianProcessInterpolatorPose3.h:57-105
Each case records its inputs, `e` (the error, or the interpolated pose), `H_ref` (what a rounding-free reference
returns: the analytic blocks exactly, the jacobianMethodNumercialDiff block -- Pose3utils.cpp:167-179 -- as the h = 1e-6
quotient with the |th| > 1e-5 branch of rightJacobianPose3Q, Pose3utils.cpp:92-113), `H_exact` (the derivative of the same
e, central difference at h = 1e-20 under the right perturbations p Exp(d), v + d, in full float64 precision: the reference
of the fp32 rows, which do not restate the quotient -- tests/test_gpu_fp32_rows.py), `H_ref_minus_exact` (H_ref minus it, to
three digits) and theta = |Log(T1^-1 T2)| of the rotation part.  For 5e-6 < th < 2e-3 a case also holds `e64` / `H_ref64`: the same with rightJacobianPose3Q's
closed-form coefficients as float64 forms them (tests/se3_bounds.py, float64_coefficients), since there those coefficients
are all rounding and their error is as large as the branch's jump.  Whenever a quotient's rotational +-h straddles th = 1e-5, the perturbed angles stay at least 1e-12
away from it (checked below), so float64 rounding never decides the branch.

    python tests/golden/make_se3_jac_pins.py
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import se3_bounds as B  # noqa: E402

mp.mp.dps = 50
B.M = mp

THETAS = [0.0, 1e-9, 1e-6, 9.5e-6, 1.05e-5, 3e-5, 1e-4, 1e-3, 1e-2, 0.3, 1.5, 3.0, float(mp.pi) - 1e-3]
TAUS = [0.3, 1.0, -0.1, 1.1]
QC = [[0.01, 0.003, 0.0, 0.0, 0.0, 0.001], [0.003, 0.02, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.015, 0.002, 0.0, 0.0],
      [0.0, 0.0, 0.002, 0.01, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.02, 0.0], [0.001, 0.0, 0.0, 0.0, 0.0, 0.03]]
DT = 0.1
H_EX = mp.mpf(10) ** -20


def fl(x):
    v = float(x)
    return 0.0 if abs(v) < 1e-30 else v        # exact zeros carry 50-digit residue of 1e-50 .. 1e-30: written as 0


def f64(v):
    return [fl(x) for x in v]


def mpv(v):
    return [mp.mpf(float(x)) for x in v]


def fmat(Mx):
    return [[fl(x) for x in row] for row in Mx]


def diff3(H, Hx):
    """H_ref - H_exact to three digits (the record of the jump at 1e-5 and of the h^2 / 6 truncation)"""
    return [[[float("%.3g" % float(a - b)) for a, b in zip(r, s)] for r, s in zip(h, hx)] for h, hx in zip(H, Hx)]


def retract(p, d):
    return B.compose(p, B.pose3_expmap(d))


def rand_pose(rng, scale=1.0):
    w = rng.standard_normal(3)
    return f64(B.pose3_expmap(mpv(list(w)) + mpv(list(scale * rng.standard_normal(3)))))


def straddle_ok(r):
    """every rotational +-h of the quotient is >= 1e-12 from the 1e-5 branch point"""
    for k in range(3):
        for s in (1, -1):
            w = [r[i] + (s * mp.mpf(B.H_FD) if i == k else 0) for i in range(3)]
            if abs(mp.sqrt(sum(x * x for x in w)) - mp.mpf(1e-5)) < 1e-12:
                return False
    return abs(mp.sqrt(sum(x * x for x in r[:3])) - mp.mpf(1e-5)) >= 1e-12


def straddles(r):
    th = [mp.sqrt(sum((r[i] + (s * mp.mpf(B.H_FD) if i == k else 0)) ** 2 for i in range(3)))
          for k in range(3) for s in (1, -1)]
    return any(t > 1e-5 for t in th) and any(t <= 1e-5 for t in th)


def make_pair(rng, theta, rho_scale, axis=None):
    p1 = rand_pose(rng, 2.0)
    ax = np.asarray(axis if axis is not None else rng.standard_normal(3), dtype=float)
    ax = ax / np.linalg.norm(ax)
    rho = rng.standard_normal(3)
    rho = rho_scale * rho / np.linalg.norm(rho)
    xi = list(theta * ax) + list(rho)
    p2 = f64(retract(mpv(p1), mpv(xi)))
    return p1, p2


def model64(case, fn):
    """the float64-coefficient pins (se3_bounds.float64_coefficients) where the closed forms of rightJacobianPose3Q are
    all rounding: 5e-6 < th < 2e-3"""
    if 5e-6 < case["theta"] < 2e-3:
        with B.float64_coefficients():
            e, H, _ = fn()
        case["e64"], case["H_ref64"] = f64(e), [fmat(h) for h in H]
    return case


def gp_case(rng, theta, rho_scale, axis=None, note=""):
    for _ in range(20):
        p1, p2 = make_pair(rng, theta, rho_scale, axis)
        v1, v2 = f64(rng.standard_normal(6)), f64(rng.standard_normal(6))
        e, H, r = B.gp_prior(mpv(p1), mpv(v1), mpv(p2), mpv(v2), mp.mpf(DT))
        if straddle_ok(r):
            break
    else:
        raise RuntimeError("no case clear of the branch point at theta %g" % theta)

    def err(d):
        q1 = retract(mpv(p1), d[0:6])
        q2 = retract(mpv(p2), d[12:18])
        w1 = [mp.mpf(v1[i]) + d[6 + i] for i in range(6)]
        w2 = [mp.mpf(v2[i]) + d[18 + i] for i in range(6)]
        return B.gp_prior(q1, w1, q2, w2, mp.mpf(DT))[0]

    Hx = [[[0] * 6 for _ in range(12)] for _ in range(4)]
    for m in range(4):
        for k in range(6):
            d = [mp.mpf(0)] * 24
            d[6 * m + k] = H_EX
            ep = err(d)
            d[6 * m + k] = -H_EX
            en = err(d)
            for i in range(12):
                Hx[m][i][k] = (ep[i] - en[i]) / (2 * H_EX)
    th = mp.sqrt(sum(x * x for x in r[:3]))
    case = dict(family="gp_prior_pose3", src="gpslam/gp/GaussianProcessPriorPose3.h:60-98; Pose3utils.cpp:92-113,167-179",
                note=note, p1=p1, v1=v1, p2=p2, v2=v2, dt=DT, theta=float(th), straddles=bool(straddles(r)),
                rho=float(mp.sqrt(sum(x * x for x in r[3:]))),
                e=f64(e), H_ref=[fmat(h) for h in H], H_ref_minus_exact=diff3(H, Hx), H_exact=[fmat(h) for h in Hx])
    return model64(case, lambda: B.gp_prior(mpv(p1), mpv(v1), mpv(p2), mpv(v2), mp.mpf(DT)))


def lam_psi(dt, tau):
    Qc = mp.matrix(QC)

    def Qm(t):
        Q = mp.zeros(12, 12)
        for i in range(6):
            for j in range(6):
                Q[i, j] = t ** 3 / 3 * Qc[i, j]
                Q[i, 6 + j] = Q[6 + i, j] = t ** 2 / 2 * Qc[i, j]
                Q[6 + i, 6 + j] = t * Qc[i, j]
        return Q

    def Phi(t):
        P = mp.eye(12)
        for i in range(6):
            P[i, 6 + i] = t
        return P

    dt, tau = mp.mpf(dt), mp.mpf(tau)
    Psi = Qm(tau) * Phi(dt - tau).T * Qm(dt) ** -1          # GPutils.cpp calcPsi
    Lam = Phi(tau) - Psi * Phi(dt)                          # calcLambda
    return [[Lam[i, j] for j in range(12)] for i in range(12)], [[Psi[i, j] for j in range(12)] for i in range(12)]


def interp_case(rng, theta, rho_scale, tau_frac, axis=None, note=""):
    tau = tau_frac * DT
    Lam, Psi = lam_psi(DT, tau)
    for _ in range(20):
        p1, p2 = make_pair(rng, theta, rho_scale, axis)
        v1, v2 = f64(rng.standard_normal(6)), f64(rng.standard_normal(6))
        out, H, r = B.interpolate(Lam, Psi, mpv(p1), mpv(v1), mpv(p2), mpv(v2))
        if straddle_ok(r):
            break
    else:
        raise RuntimeError("no case clear of the branch point at theta %g" % theta)
    inv0 = B.inverse(out)

    def pose_at(d):
        q1 = retract(mpv(p1), d[0:6])
        q2 = retract(mpv(p2), d[12:18])
        w1 = [mp.mpf(v1[i]) + d[6 + i] for i in range(6)]
        w2 = [mp.mpf(v2[i]) + d[18 + i] for i in range(6)]
        return B.interpolate(Lam, Psi, q1, w1, q2, w2)[0]

    Hx = [[[0] * 6 for _ in range(6)] for _ in range(4)]
    for m in range(4):
        for k in range(6):
            d = [mp.mpf(0)] * 24
            d[6 * m + k] = H_EX
            lp = B.pose3_logmap(B.compose(inv0, pose_at(d)))
            d[6 * m + k] = -H_EX
            ln = B.pose3_logmap(B.compose(inv0, pose_at(d)))
            for i in range(6):
                Hx[m][i][k] = (lp[i] - ln[i]) / (2 * H_EX)
    th = mp.sqrt(sum(x * x for x in r[:3]))
    case = dict(family="interpolate_pose3", src="gpslam/gp/GaussianProcessInterpolatorPose3.h:57-105; Pose3utils.cpp:92-113,167-179",
                note=note, p1=p1, v1=v1, p2=p2, v2=v2, dt=DT, tau=tau, theta=float(th), straddles=bool(straddles(r)),
                rho=float(mp.sqrt(sum(x * x for x in r[3:]))),
                e=f64(out), H_ref=[fmat(h) for h in H], H_ref_minus_exact=diff3(H, Hx), H_exact=[fmat(h) for h in Hx])
    return model64(case, lambda: B.interpolate(Lam, Psi, mpv(p1), mpv(v1), mpv(p2), mpv(v2)))


def main():
    rng = np.random.default_rng(20261016)
    gp, it = [], []
    for th in THETAS:
        gp.append(gp_case(rng, th, 0.6))
        it.append(interp_case(rng, th, 0.6, TAUS[len(it) % 4]))
        if th >= 1e-6:
            gp.append(gp_case(rng, th, 10.0, note="|rho| = 10"))
    # the quotient's rotational +-h across the 1e-5 branch point: rotation axis close to e_x
    for th in (9.5e-6, 1.05e-5):
        gp.append(gp_case(rng, th, 0.6, axis=[1.0, 0.02, -0.03], note="+-h straddles 1e-5"))
        it.append(interp_case(rng, th, 0.6, TAUS[len(it) % 4], axis=[1.0, 0.02, -0.03], note="+-h straddles 1e-5"))
    for tf in TAUS:
        it.append(interp_case(rng, 0.3, 10.0, tf, note="|rho| = 10"))
    assert any(c["straddles"] for c in gp) and any(c["straddles"] for c in it)
    pins = dict(note="mpmath %s, %d digits; generated by tests/golden/make_se3_jac_pins.py" % (mp.__version__, mp.mp.dps),
                h_fd=B.H_FD, Qc=QC, gp_prior_pose3=gp, interpolate_pose3=it)
    # `H_exact` goes to a file of its own, one case per line, so that se3_jac_pins.json stays byte for byte what it was
    # (a block that equals the case's H_ref block bit for bit -- the GP prior's analytic H2 and H4 -- is written as null)
    exact = {fam: [[None if hx == h else hx for hx, h in zip(c.pop("H_exact"), c["H_ref"])] for c in pins[fam]]
             for fam in ("gp_prior_pose3", "interpolate_pose3")}
    path = os.path.join(HERE, "se3_jac_pins.json")
    with open(path, "w") as f:
        json.dump(pins, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")
    path = os.path.join(HERE, "se3_jac_pins_exact.json")
    with open(path, "w") as f:
        f.write('{"note":"H_exact of every case of se3_jac_pins.json, in its order; generated with it; null: the block equals that of H_ref bit for bit"')
        for fam, hs in exact.items():
            f.write(',\n"%s":[\n%s\n]' % (fam, ",\n".join(json.dumps(h, separators=(",", ":")) for h in hs)))
        f.write("}\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
