"""CPU side of tests/test_gpu_fp32_rows.py: every reference that file holds the fp32 rows to is checked here against the oracle, and
the side conditions of its graphs are measured.  Each check also fails for a deliberately wrong reference.

Figures (printed by the tests): consecutive relative rotations of the POSE3 measurement graphs 0.416 .. 1.106 rad, of the projection
graph 0.446 .. 1.085 rad; smallest ranged distance 5.42 m (pose3), 5.47 m (pose3+sensor), 4.57 m (pose2, pose2+sensor), 2.41 m
(linear3); 100 eps kappa_s of the step graphs 1.8e-9 (SE(3) chain), 1.7e-9 (SE(2) chain), 4.5e-8 and 4.3e-8 (4 and 11 landmarks),
1.2e-10 (SE(3) + interpolated GPS); GPS rows from the pins against the oracle 0.33 of the 1e-7 bound."""
import hashlib
import json
import os

import numpy as np
import pytest

import fp32_rows_refs as R
import rows_model as RM
from oracle import oracle as O

# sha256 of the fixture (json.dumps(sort_keys=True, separators=(",", ":")) of the whole file)
PINS_DIGEST_WITHOUT_H_EXACT = "1bcc0f24eef4a1ed0e2a6754fbf3f7362f344e8a5cc9f992cccfbe883b31e877"


@pytest.fixture(scope="module")
def pins():
    return R.load_pins()


def test_the_pins_fixture_itself_is_unchanged():
    """`H_exact` lives in se3_jac_pins_exact.json: the fixture the fp64 suites read has the content it had"""
    with open(os.path.join(R.HERE, "golden", "se3_jac_pins.json")) as f:
        p = json.load(f)
    assert not any("H_exact" in c for fam in ("gp_prior_pose3", "interpolate_pose3") for c in p[fam])
    got = hashlib.sha256(json.dumps(p, sort_keys=True, separators=(",", ":")).encode()).hexdigest()
    assert got == PINS_DIGEST_WITHOUT_H_EXACT
    q = R.load_pins()
    assert sum("H_exact" in c for fam in ("gp_prior_pose3", "interpolate_pose3") for c in q[fam]) == 26 + 19
    assert os.path.getsize(os.path.join(R.HERE, "golden", "se3_jac_pins_exact.json")) < 1 << 20


def test_h_exact_is_the_derivative_the_recorded_difference_was_taken_from(pins):
    """H_ref - H_exact reproduces the three-digit H_ref_minus_exact of every case, up to the float64 rounding of the two stored values"""
    for c in pins["gp_prior_pose3"] + pins["interpolate_pose3"]:
        Href, Hx, dif = np.asarray(c["H_ref"]), np.asarray(c["H_exact"]), np.asarray(c["H_ref_minus_exact"])
        assert Hx.shape == Href.shape
        slack = 0.006 * np.abs(dif) + 4 * RM.EPS * np.abs(Href) + 1e-30
        assert (np.abs(Href - Hx - dif) <= slack).all(), (c["family"], c["theta"], c["note"])


def oracle_gps(pins):
    fl = R.gps_graph(pins)
    orc = fl.replay(O.Chain(O.POSE3))
    n = len(pins["interpolate_pose3"])
    return orc.linearize_meas(3, n)


def gps_mismatch(pins, rows, e0, J0):
    """largest |reference from the pins - oracle| over the pins with theta >= 0.3, in units of the 1e-7 max(1, |J|max) that
    test_measurement_factors_per_factor_error_and_jacobians gives rows through the h = 1e-6 quotient.  (The errors, -offset in exact
    arithmetic, at 1e-10: at theta = pi - 1e-3 the oracle's interpolated translation carries Logmap's conditioning 1 / (pi - theta).)"""
    worst, n = 0.0, 0
    for k, c in enumerate(pins["interpolate_pose3"]):
        if c["theta"] < 0.3:
            continue
        J, e = rows[k]
        worst = max(worst, np.abs(J - J0[k][:, :24]).max() / (1e-7 * max(1.0, np.abs(J0[k]).max())), np.abs(e - e0[k]).max() / 1e-10)
        n += 1
    assert n >= 8
    return worst


def test_gps_rows_from_the_pins_match_the_oracle(pins):
    e0, J0 = oracle_gps(pins)
    rows = R.gps_rows(pins, whiten=False)
    worst = gps_mismatch(pins, rows, e0, J0)
    print("GPS rows from the pins against the oracle's linearize_meas, theta >= 0.3: worst / 1e-7 = %.3g" % worst)
    assert worst <= 1.0
    assert np.abs(J0[:, :, 24:]).max() == 0.0
    # whitening: 1 / sigma per axis
    for (Jw, ew), (J, e) in zip(R.gps_rows(pins), rows):
        assert np.allclose(Jw * R.GPS_SIGMA[:, None], J, rtol=1e-15, atol=0) and np.allclose(ew * R.GPS_SIGMA, e, rtol=1e-15, atol=0)


def test_gps_row_check_fails_for_a_wrong_reference(pins):
    """one pin's H_exact block negated, the rotation left out, or the rotational rows taken: each is seen"""
    e0, J0 = oracle_gps(pins)
    k = next(i for i, c in enumerate(pins["interpolate_pose3"]) if c["theta"] >= 0.3)
    bad = json.loads(json.dumps(pins))
    bad["interpolate_pose3"][k]["H_exact"][2] = (-np.asarray(pins["interpolate_pose3"][k]["H_exact"][2])).tolist()
    assert gps_mismatch(bad, R.gps_rows(bad, whiten=False), e0, J0) > 1e3
    no_rot = [(np.hstack([np.asarray(h)[3:6, :] for h in c["H_exact"]]), -R.GPS_OFFSET) for c in pins["interpolate_pose3"]]
    assert gps_mismatch(pins, no_rot, e0, J0) > 1e3
    rot_rows = [(np.hstack([np.asarray(c["e"])[:9].reshape(3, 3) @ np.asarray(h)[0:3, :] for h in c["H_exact"]]), -R.GPS_OFFSET)
                for c in pins["interpolate_pose3"]]
    assert gps_mismatch(pins, rot_rows, e0, J0) > 1e3


def test_gp_prior_rows_from_the_pins_match_the_oracle_where_the_quotient_is_a_derivative(pins):
    """0.2 < theta < 1.5: R_w H_exact against the oracle's whitened rows (through the normal equations of one factor: D = J^T J)"""
    rows = R.gp_prior_rows(pins)
    n = 0
    for k, c in enumerate(pins["gp_prior_pose3"]):
        if not 0.2 < c["theta"] < 1.5:
            continue
        orc = O.Chain(O.POSE3)
        orc.set_qc(np.asarray(pins["Qc"]))
        orc.set_states(np.array([c["p1"], c["p2"]]), np.array([c["v1"], c["v2"]]))
        orc.add_gp_priors([0], [c["dt"]])
        D, Om, g, _, _, _ = orc.normal_equations()
        J, e = rows[k]
        JL, JR = J[:, :12], J[:, 12:]
        H = np.block([[JL.T @ JL, JL.T @ JR], [JR.T @ JL, JR.T @ JR]])
        H0 = np.block([[D[0], Om[0].T], [Om[0], D[1]]])
        assert np.abs(H - H0).max() <= 1e-5 * np.abs(H0).max(), (c["theta"], c["note"])
        g0 = np.concatenate([g[0], g[1]])
        assert np.abs(-J.T @ e - g0).max() <= 1e-5 * np.abs(g0).max(), (c["theta"], c["note"])
        n += 1
    assert n >= 2


# ---------------------------------------------------------------- the translated twin of a graph

def translatable_graphs():
    from test_gpu_measurements import meas_graph, LD
    from test_gpu_projection import build_pair
    out = []
    for name, (kind, sensor) in R.meas_cases():
        if R.trans_slice(kind) is None:
            continue
        feed, _ = meas_graph(kind, sensor=sensor, **R.meas_kwargs(kind))
        chart = O.CHART_FIRST_ORDER if kind == O.POSE2 else O.CHART_EXPMAP
        out.append((name, kind, chart, LD[kind], feed(RM.FactorLists(O.TANGENT_DIM[kind], LD[kind]))))
    out.append(("linear2", O.LINEAR2, O.CHART_EXPMAP, 0, R.linear2_feed()(RM.FactorLists(2))))
    (fl,), _ = build_pair(motion=R.MOTION3, makers=(lambda: RM.FactorLists(6, 3),))
    out.append(("projection", O.POSE3, O.CHART_EXPMAP, 3, fl))
    return out


@pytest.fixture(scope="module")
def graphs():
    return translatable_graphs()


def test_translated_twin_has_the_same_error_on_the_oracle(graphs):
    """every factor is invariant under the common translation: the oracle's error moves by fp64 rounding at 1e5 m only -- and moves
    visibly when one moved quantity is left behind (the GPS measurements, the landmark priors)"""
    for name, kind, chart, ld, fl in graphs:
        T = R.world_shift(kind)
        e0 = fl.replay(O.Chain(kind, chart, ld)).error()
        e1 = fl.replay(O.Chain(kind, chart, ld), edit=R.translate(kind, T)).error()
        print("%s: error %.12g, translated %.12g" % (name, e0, e1))
        assert abs(e0 - e1) <= 1e-8 * e0, name
        full = R.translate(kind, T)
        for left_out in ("add_interp_gps", "add_landmark_priors", "add_pose_priors"):
            if not fl.args_of(left_out):
                continue
            e2 = fl.replay(O.Chain(kind, chart, ld), edit=lambda n, a: a if n == left_out else full(n, a)).error()
            assert abs(e0 - e2) > 1e3 * e0, (name, left_out)


def test_side_conditions_of_the_measurement_graphs(graphs):
    """consecutive relative rotations of every SE(3) graph in (0.2, 1.5) rad; every ranged landmark >= 0.5 m away"""
    seen = 0
    for name, kind, chart, ld, fl in graphs:
        if kind == O.POSE3:
            th = R.relative_rotations(fl.args_of("set_states")[0][0])
            print("%s: relative rotations %.3f .. %.3f rad" % (name, th.min(), th.max()))
            assert 0.2 < th.min() and th.max() < 1.5, name
            seen += 1
        if fl.args_of("add_interp_range") or fl.args_of("add_bearing_range"):
            dist = R.ranged_distances(kind, fl)
            print("%s: ranged distances >= %.2f m (%d factors)" % (name, dist.min(), len(dist)))
            assert dist.min() >= 0.5 and len(dist) >= 100, name
            seen += 1
    assert seen == 3 + 5


# ---------------------------------------------------------------- the step comparison

@pytest.mark.parametrize("form", R.step_forms(), ids=[f[0] for f in R.step_forms()])
def test_step_graphs_are_conditioned_for_the_bound_and_the_update_is_recovered(form):
    """per graph of the step comparison, on the oracle: 100 eps kappa_s <= 1e-7 (rows_model.step_tol asserts it), and the update
    recovered from the states of one iterate_gn equals the dense solve of the oracle's own normal equations within that bound"""
    id, recipe, dev, _ = form
    kind, chart, feed = recipe()
    ld = dev.get("landmark_dim", 0)
    orc = feed(O.Chain(kind, chart, ld))
    D, Om, g, B, HLL, gL = orc.normal_equations()
    H = RM.dense(D, Om, B, HLL)
    rhs = g.ravel() if B is None else np.concatenate([g.ravel(), gL])
    tol = RM.step_tol(H)
    print("%s: kappa_s %.3g, 100 eps kappa_s %.3g" % (id, RM.scaled_cond(H), 100 * RM.EPS * RM.scaled_cond(H)))
    before, lm0 = orc.get_states(), (orc.get_landmarks() if ld else None)
    rc, _ = orc.iterate_gn()
    assert rc == 0
    dx = R.update_of(kind, chart, before, orc.get_states(), lm0, orc.get_landmarks() if ld else None)
    dx_ref = np.linalg.solve(H, rhs)
    r = R.scaled_step_difference(H, dx_ref, dx)
    print("%s: scaled step difference %.3g (bound %.3g)" % (id, r, tol))
    assert r <= tol
    # a wrong sign of the right-hand side, or the landmark part dropped, is far outside
    assert R.scaled_step_difference(H, -dx_ref, dx) > 1.0


def test_inside_the_references_flat_branch_the_derivative_is_the_quotient_pin(pins):
    """th^2 <= eps (the pins at 0 and 1e-9): H_exact, a difference at h = 1e-20 inside the branch where rightJacobianRot3inv is I, misses
    the rotation coupling by O(1) and fp32_rows_refs.exact_derivative takes H_ref; next to the branch (th = 1e-6) the two agree to
    1e-11, so nothing else changes.  With H_ref the GPS rows of those pins match the oracle like the large rotations do."""
    inside = outside = 0
    for c in pins["gp_prior_pose3"] + pins["interpolate_pose3"]:
        d = np.abs(np.asarray(c["H_ref"]) - np.asarray(c["H_exact"])).max()
        if c["theta"] ** 2 <= RM.EPS:
            assert d > 0.05 and R.exact_derivative(c) is c["H_ref"], (c["family"], c["theta"], d)
            inside += 1
        else:
            assert R.exact_derivative(c) is c["H_exact"]
            if c["theta"] < 2e-6:
                assert d < 1e-11, (c["family"], c["theta"], d)
                outside += 1
    assert inside == 4 and outside >= 3
    e0, J0 = oracle_gps(pins)
    rows = R.gps_rows(pins, whiten=False)
    for k, c in enumerate(pins["interpolate_pose3"]):
        if c["theta"] ** 2 <= RM.EPS:
            assert np.abs(rows[k][0] - J0[k][:, :24]).max() <= 1e-7 * max(1.0, np.abs(J0[k]).max()), c["theta"]
