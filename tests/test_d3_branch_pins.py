"""tests/golden/d3_branch_pins.json on the CPU: the oracle against every 50-digit pin of the SE(2) / SO(3) factors, and the
conditions that make those pins a yardstick (tests/golden/make_d3_branch_pins.py) re-asserted from the file alone.

The tolerance of the device tests is 8 noise + 8 u |exact| per entry, `noise` being the oracle's own error against its formula in
exact arithmetic over the case and 32 neighbours.  Here the oracle itself is held to noise + 8 u |exact| at the case."""
import numpy as np
import pytest

import d3_branch_refs as D


@pytest.fixture(scope="module")
def pins():
    return D.load_pins()


def test_the_file_is_no_larger_than_the_se3_pins(pins):
    import os
    g = os.path.join(D.HERE, "golden")
    assert os.path.getsize(os.path.join(g, "d3_branch_pins.json")) <= 327991        # se3_jac_pins.json when these pins were added
    assert set(pins["families"]) == set(D.FAMILIES)


@pytest.mark.parametrize("fam", sorted(D.FAMILIES))
def test_oracle_within_its_noise_of_every_pin(pins, fam):
    worst = 0.0
    for k, c in enumerate(pins["families"][fam]):
        got, pin = D.oracle_eval(fam, c["inputs"], pins["Qc"]), D.pin_of(c)
        assert got.shape == pin.shape == (len(c["noise"]),)
        bound = np.asarray(c["noise"]) + 8 * D.U * np.abs(pin)
        d = np.abs(got - pin)
        assert (d <= bound).all(), (fam, k, c["label"], float((d - bound).max()))
        worst = max(worst, float((d / (bound + 1e-300)).max()))
    print("%s: oracle / (noise + 8 u |exact|), worst %.3g" % (fam, worst))


def test_no_case_is_meaningless_and_tol_max_is_what_the_entries_give(pins):
    for fam, cases in pins["families"].items():
        for k, c in enumerate(cases):
            tol = D.tol_of(c)
            assert tol.max() <= pins["tol_limit"] == 1e-5, (fam, k, c["label"], tol.max())
            assert abs(tol.max() - c["tol_max"]) <= 0.006 * tol.max(), (fam, k)       # (written to three digits)


def test_conditions_on_the_decides_data_hold(pins):
    """every side that some case decides has a deciding case (>= 100 tol to the other branch's exact value) in every family that
    reaches it; every branch the Lie maps have is taken; the table and the undecidable sides in the file are what the cases give"""
    assert pins["decides_at"] == 100
    table, undecidable, problems = D.conditions(pins["families"], pins["named_branches"], pins["decides_at"])
    assert not problems, problems
    assert undecidable == pins["undecidable"]
    assert len(table) == len(pins["table"])
    for a, b in zip(table, pins["table"]):
        for key in ("function", "branch", "side", "decided", "deciding_cases", "value_check_only_at"):
            assert a[key] == b[key], (a, b)
    # a side that nothing decides at all would be a value check only: few, and only ever because the two branches agree to rounding
    assert len(undecidable) <= 4
    # where a decided side is a value check only, it is just above a small-angle threshold or on the small side of one
    for row in table:
        assert all(abs(a) <= 1e-7 for a in row["value_check_only_at"]), row


def test_every_named_branch_and_threshold_side_is_in_the_grid(pins):
    named = {tuple(nb) for nb in pins["named_branches"]}
    # SE(2): both sides of 1e-10 (Log, Exp) and of 1e-5 (dexp, dlog), wrap_pi wrapping; SO(3): both sides of th^2 = eps, the three
    # Logmap branches and the three sub-branches of the window at pi
    for need in [("se2_log", "first_order"), ("se2_log", "closed"), ("se2_exp", "first_order"), ("se2_exp", "closed"),
                 ("se2_dexp", "series"), ("se2_dexp", "closed"), ("se2_dlog", "series"), ("se2_dlog", "closed"), ("wrap_pi", "wraps"),
                 ("so3_exp", "first_order"), ("so3_exp", "rodrigues"), ("so3_jr", "identity"), ("so3_jr", "closed"),
                 ("so3_jrinv", "identity"), ("so3_jrinv", "closed"), ("so3_log", "series"), ("so3_log", "acos"),
                 ("so3_log", "pi_z"), ("so3_log", "pi_y"), ("so3_log", "pi_x")]:
        assert need in named, need
    fams = pins["families"]
    for fam, cases in fams.items():
        kind = D.FAMILIES[fam][0]
        angles = {c["angle"] for c in cases}
        if kind == D.O.POSE2:
            assert {0.0, 5e-11, -5e-11, 2e-10, 1e-7, 5e-6, 2e-5, 1e-3, 0.3, 3.0, np.pi - 1e-6, np.pi} <= angles, fam
            assert sum(abs(abs(a) - (2 * np.pi - 0.1)) < 1e-12 for a in angles) == 2, fam
            assert any(c["angle"] == 0.0 and c["scale"] == 0.0 for c in cases) and any(c["angle"] == 0.0 and c["scale"] > 0 for c in cases)
        else:
            assert {0.0, 1e-9, 1e-8, 2e-8, 2e-4, 5e-4, 0.3, 3.0, np.pi - 1e-3, np.pi - 2e-5, np.pi - 5e-6, np.pi} <= angles, fam
            assert {c["taken"]["so3_log"] for c in cases if c["angle"] == np.pi} == {"pi_z", "pi_y", "pi_x"}, fam
    # the stationary case is an all-zero interval: equal poses, zero velocities
    for fam in ("gp_prior_pose2", "gp_prior_rot3", "interp_pose2", "interp_rot3"):
        c = [c for c in fams[fam] if c["angle"] == 0.0 and c["scale"] == 0.0][0]["inputs"]
        assert c["p1"] == c["p2"] and not any(c["v1"]) and not any(c["v2"]), fam


@pytest.mark.parametrize("kind,chart", [(D.O.POSE2, D.O.CHART_FIRST_ORDER), (D.O.POSE2, D.O.CHART_EXPMAP), (D.O.ROT3, D.O.CHART_EXPMAP)],
                         ids=["pose2-first-order", "pose2-expmap", "rot3"])
def test_edge_chain_twin_lands_within_1e_10(pins, kind, chart):
    """tests/d3_edge_chain.py: the oracle and its twin started 1e-15 away stay within 1e-10 (relative) over the one and the two
    Gauss-Newton steps the GPU test takes, so the 1e-9 of the per-step rule hides nothing on this chain; and the chain's intervals
    take the small-angle branches, the straight and the stationary interval among them."""
    import d3_edge_chain as E
    cases = E.chain_cases(pins, kind)
    assert all(c["tol_max"] <= 1e-11 for c in cases) and len(cases) >= 8
    # every deciding GP-prior case with tol <= 1e-11 is in the chain, but for SE(2)'s intervals of pi exactly (on the cut of wrap_pi)
    fam = pins["families"][E.FAMILY[kind]]
    left_out = [c for c in fam if c["tol_max"] <= 1e-11 and max(c["decides"].values(), default=0.0) >= 100 and c not in cases]
    assert all(kind == D.O.POSE2 and c["angle"] == np.pi for c in left_out) and len(left_out) == (3 if kind == D.O.POSE2 else 0), left_out
    _, _, taken = E.recipe(pins, kind, chart)
    need = (["se2_log:first_order", "se2_log:closed", "se2_dlog:series", "se2_dlog:closed", "wrap_pi:wraps"] if kind == D.O.POSE2 else
            ["so3_log:series", "so3_log:acos", "so3_log:pi_z", "so3_log:pi_y", "so3_log:pi_x", "so3_jrinv:identity", "so3_jrinv:closed"])
    assert set(need) <= set(taken), taken
    for steps in (1, 2):
        _, s0, dist = E.oracle_and_twin(pins, kind, chart, steps)
        print("%d step(s): cost %.6g -> %.6g, twin distance (error_before, error_after, poses, velocities) %s" % (
            steps, s0.error_before, s0.error_after, ["%.2e" % v for v in dist]))
        assert dist.max() < 1e-10, dist
