"""The HIP kernels against the 50-digit SE(3) Jacobian pins (tests/golden/se3_jac_pins.json), each entry within the
float64 rounding bound of tests/se3_bounds.py.  Every case of one family sits in one handle, as 2K states with the
factor (or the interpolation) on (2k, 2k+1), so one wave mixes branches and rotation scales.  The kernel forms the
translational columns of the h = 1e-6 quotient in closed form (gpslam_amd/csrc/factors.hpp): they are held to the
bound of that closed form, since in exact arithmetic it equals the quotient."""
import json
import os

import numpy as np
import pytest

import se3_bounds as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(HERE, "golden", "se3_jac_pins.json")) as f:
        return json.load(f)


def ratio(got, ref, bound):
    got, ref = np.asarray(got), np.asarray(ref)
    return (np.abs(got - ref) / (bound + 2 * B.U * np.abs(ref) + 1e-300)).max()


def solver(pins, cases, plan=0):
    import gpslam_amd
    s = gpslam_amd.ChainSolver(O.POSE3, O.CHART_EXPMAP, plan=plan)
    s.set_qc(np.asarray(pins["Qc"]))
    pose = np.array([p for c in cases for p in (c["p1"], c["p2"])])
    vel = np.array([v for c in cases for v in (c["v1"], c["v2"])])
    s.set_states(pose, vel)
    s.add_gp_priors(np.arange(0, 2 * len(cases), 2), [c["dt"] for c in cases])
    s.compile()
    return s


def test_linearize_gp_pose3_within_bound(pins):
    cases = pins["gp_prior_pose3"]
    e, H = solver(pins, cases).linearize_gp()
    worst = {}
    for k, c in enumerate(cases):
        eb, Hb = B.gp_prior_bound(c["p1"], c["v1"], c["p2"], c["v2"], c["dt"], closed=True)
        r = max(ratio(e[k], c["e"], eb), ratio(H[k], c["H_ref"], Hb))
        assert r <= 1.0, (k, c["theta"], c["note"], r)
        key = "%.3g" % c["theta"]
        worst[key] = max(worst.get(key, 0.0), float(r))
    print("linearize_gp device / bound by theta:", worst)


def test_interpolate_poses_jac_pose3_within_bound(pins):
    cases = pins["interpolate_pose3"]
    Qc = np.asarray(pins["Qc"])
    s = solver(pins, cases)
    left = np.arange(0, 2 * len(cases), 2).astype(np.int32)
    out, H = s.interpolate_poses_jac(left, [c["dt"] for c in cases], [c["tau"] for c in cases])
    worst = {}
    for k, c in enumerate(cases):
        Lam, Psi = O.lambda_psi(6, Qc, c["dt"], c["tau"])
        cond = B.lambda_psi_cond(c["dt"]) * float(np.linalg.cond(Qc))
        ob, Hb = B.interpolate_bound(Lam, Psi, c["p1"], c["v1"], c["p2"], c["v2"], closed=True, cond=cond)
        r = max(ratio(out[k], c["e"], ob), ratio(H[k], c["H_ref"], Hb))
        assert r <= 1.0, (k, c["theta"], c["tau"], c["note"], r)
        key = "%.3g" % c["theta"]
        worst[key] = max(worst.get(key, 0.0), float(r))
    print("interpolate_poses_jac device / bound by theta:", worst)


def test_branch_side_against_float64_coefficient_pins(pins):
    """5e-6 < th < 2e-3, the straddling quotients among them: k_gp and interpolate_poses_jac against H_ref64, the pins
    with rightJacobianPose3Q's closed-form coefficients as float64 forms them (tests/se3_bounds.py).  The bound left
    without the coefficients' rounding is far below the jump of the branch at 1e-5, so a kernel that takes the other
    side of 1e-5 anywhere in a quotient fails here."""
    Qc = np.asarray(pins["Qc"])
    gp = pins["gp_prior_pose3"]
    e, H = solver(pins, gp).linearize_gp()
    it = pins["interpolate_pose3"]
    out, Hi = solver(pins, it).interpolate_poses_jac(np.arange(0, 2 * len(it), 2).astype(np.int32),
                                                   [c["dt"] for c in it], [c["tau"] for c in it])
    worst, n = {}, 0
    with B.float64_coefficients():
        for k, c in enumerate(gp):
            if "H_ref64" in c:
                eb, Hb = B.gp_prior_bound(c["p1"], c["v1"], c["p2"], c["v2"], c["dt"], closed=True)
                r = max(ratio(e[k], c["e64"], eb), ratio(H[k], c["H_ref64"], Hb))
                assert r <= 1.0, ("gp_prior", c["theta"], c["note"], r)
                worst["gp %.3g" % c["theta"]] = max(worst.get("gp %.3g" % c["theta"], 0.0), float(r))
                n += 1
        for k, c in enumerate(it):
            if "H_ref64" in c:
                Lam, Psi = O.lambda_psi(6, Qc, c["dt"], c["tau"])
                cond = B.lambda_psi_cond(c["dt"]) * float(np.linalg.cond(Qc))
                ob, Hb = B.interpolate_bound(Lam, Psi, c["p1"], c["v1"], c["p2"], c["v2"], closed=True, cond=cond)
                r = max(ratio(out[k], c["e64"], ob), ratio(Hi[k], c["H_ref64"], Hb))
                assert r <= 1.0, ("interpolate", c["theta"], c["tau"], c["note"], r)
                worst["interp %.3g" % c["theta"]] = max(worst.get("interp %.3g" % c["theta"], 0.0), float(r))
                n += 1
    assert n >= 12
    print("device / bound against the float64-coefficient pins:", worst)
