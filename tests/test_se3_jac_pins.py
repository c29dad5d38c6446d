"""The oracle against the 50-digit SE(3) Jacobian pins (tests/golden/se3_jac_pins.json, tests/golden/make_se3_jac_pins.py),
small relative rotations included, each entry within the float64 rounding bound of tests/se3_bounds.py.  This validates
the fixture and the bound together; tests/test_gpu_se3_jac_pins.py holds the HIP kernels to the same bound."""
import json
import os

import numpy as np
import pytest

import se3_bounds as B
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
BANDS = [(0.0, 1e-5, "th <= 1e-5"), (1e-5, 1e-3, "1e-5 < th < 1e-3"), (1e-3, 0.1, "1e-3 <= th < 0.1"), (0.1, 4.0, "th >= 0.1")]


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(HERE, "golden", "se3_jac_pins.json")) as f:
        return json.load(f)


def band(th):
    return next(name for lo, hi, name in BANDS if lo <= th < hi or (lo == 0.0 and th <= hi))


def within(got, ref, bound):
    """|got - ref| <= bound + the rounding of the pin itself to float64; returns the largest ratio"""
    got, ref = np.asarray(got), np.asarray(ref)
    lim = bound + 2 * B.U * np.abs(ref) + 1e-300
    return float((np.abs(got - ref) / lim).max())


def test_gp_prior_pose3_oracle_within_bound(pins):
    worst = {}
    for c in pins["gp_prior_pose3"]:
        e, H = O.gp_prior(O.POSE3, c["p1"], c["v1"], c["p2"], c["v2"], c["dt"])
        eb, Hb = B.gp_prior_bound(c["p1"], c["v1"], c["p2"], c["v2"], c["dt"])
        r = max(within(e, c["e"], eb), within(np.stack(H), c["H_ref"], Hb))
        assert r <= 1.0, (c["theta"], c["note"], r)
        worst[band(c["theta"])] = max(worst.get(band(c["theta"]), 0.0), r)
    print("gp_prior_pose3 oracle / bound:", worst)


def test_interpolate_pose3_oracle_within_bound(pins):
    Qc = np.asarray(pins["Qc"])
    worst = {}
    for c in pins["interpolate_pose3"]:
        Lam, Psi = O.lambda_psi(6, Qc, c["dt"], c["tau"])
        out, H = O.interpolate(O.POSE3, Lam, Psi, c["p1"], c["v1"], c["p2"], c["v2"])
        cond = B.lambda_psi_cond(c["dt"]) * float(np.linalg.cond(Qc))
        ob, Hb = B.interpolate_bound(Lam, Psi, c["p1"], c["v1"], c["p2"], c["v2"], cond=cond)
        r = max(within(out, c["e"], ob), within(np.stack(H), c["H_ref"], Hb))
        assert r <= 1.0, (c["theta"], c["tau"], c["note"], r)
        worst[band(c["theta"])] = max(worst.get(band(c["theta"]), 0.0), r)
    print("interpolate_pose3 oracle / bound:", worst)


def test_float64_coefficient_pins_oracle_within_bound(pins):
    """5e-6 < th < 2e-3: the closed-form coefficients of rightJacobianPose3Q are all rounding there, and their error is as
    large as the jump of the reference's branch at 1e-5, so against H_ref alone the bound cannot tell which side of 1e-5 a
    float64 evaluation took.  Against H_ref64 (those coefficients as float64 forms them, the rest in 50 digits) the bound
    without the coefficients' rounding is below 3e-7 max(1, |rho|), under the jump seen through a quotient (2e-6 .. 6e-5,
growing with |rho| as well), for the GP prior.  (For interpolatePose the Expmap of a small argument keeps
    some interpolated cases' bound larger.)"""
    Qc = np.asarray(pins["Qc"])
    n, worst = 0, {}
    with B.float64_coefficients():
        for c in pins["gp_prior_pose3"] + pins["interpolate_pose3"]:
            if "H_ref64" not in c:
                continue
            n += 1
            if c["family"] == "gp_prior_pose3":
                e, H = O.gp_prior(O.POSE3, c["p1"], c["v1"], c["p2"], c["v2"], c["dt"])
                eb, Hb = B.gp_prior_bound(c["p1"], c["v1"], c["p2"], c["v2"], c["dt"])
            else:
                Lam, Psi = O.lambda_psi(6, Qc, c["dt"], c["tau"])
                e, H = O.interpolate(O.POSE3, Lam, Psi, c["p1"], c["v1"], c["p2"], c["v2"])
                cond = B.lambda_psi_cond(c["dt"]) * float(np.linalg.cond(Qc))
                eb, Hb = B.interpolate_bound(Lam, Psi, c["p1"], c["v1"], c["p2"], c["v2"], cond=cond)
            if c["family"] == "gp_prior_pose3":
                assert Hb.max() <= 3e-7 * max(1.0, c["rho"]), (c["theta"], Hb.max())
            r = max(within(e, c["e64"], eb), within(np.stack(H), c["H_ref64"], Hb))
            assert r <= 1.0, (c["family"], c["theta"], c["note"], r)
            worst[c["family"]] = max(worst.get(c["family"], 0.0), r)
    assert n >= 12
    print("oracle / bound against the float64-coefficient pins:", worst)


def test_bound_is_not_vacuous(pins):
    """For 1e-2 <= th <= 1.5 and |rho| <= 2 the bound is no looser than the 1e-7 the suite used to hold the
    finite-difference entries (bottom rows of H1 / H3) to, and every other entry is within 1e-11, ten times below the
    1e-10 used for them.  (A rigorous bound of an h = 1e-6 quotient carries u f_abs / h = 1.1e-10 f_abs per rounding of
    each end, and at th = 1e-2 the closed forms' th^-4 cancellation on top of it: the FD entries cannot be held to 1e-9.)"""
    n = 0
    for c in pins["gp_prior_pose3"]:
        if not 1e-2 <= c["theta"] <= 1.5 or c["rho"] > 2:
            continue
        n += 1
        eb, Hb = B.gp_prior_bound(c["p1"], c["v1"], c["p2"], c["v2"], c["dt"])
        H = np.abs(np.asarray(c["H_ref"]))
        fd = np.zeros(Hb.shape, dtype=bool)
        fd[[0, 2], 6:, :] = True
        assert (Hb[fd] <= 1e-7 * np.maximum(1.0, H[fd])).all(), Hb[fd].max()
        assert Hb[~fd].max() <= 1e-11 and eb.max() <= 1e-11, (Hb[~fd].max(), eb.max())
    assert n >= 2


def test_record_reference_minus_exact(pins):
    """H_ref - H_exact: the jump of rightJacobianPose3Q at th = 1e-5 (b = +1/24 below, -1/24 above) seen by a quotient
    whose +-h straddles it, and the h^2 / 6 truncation elsewhere.  (Below th = 1e-10 Pose3::Logmap returns the
    translation itself, whose derivative misses the rotation coupling; near pi the third derivative grows.)"""
    rows = {}
    for c in pins["gp_prior_pose3"] + pins["interpolate_pose3"]:
        d = float(np.abs(np.asarray(c["H_ref_minus_exact"])).max())
        key = ("straddle " if c["straddles"] else "") + band(c["theta"])
        rows[key] = max(rows.get(key, 0.0), d)
    print("|H_ref - H_exact|:", rows)
    straddle = [v for k, v in rows.items() if k.startswith("straddle")]
    assert straddle and max(straddle) > 1e-6            # the jump over 2h: a quotient across 1e-5 is not a derivative
    assert rows["1e-3 <= th < 0.1"] < 1e-8                    # h^2 / 6 truncation + |f'''| of O(1)
