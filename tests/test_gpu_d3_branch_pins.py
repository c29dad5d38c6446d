"""The HIP kernels against the 50-digit pins of the SE(2) and SO(3) factors on every branch of their Lie maps
(tests/golden/d3_branch_pins.json; tests/golden/make_d3_branch_pins.py says how a pin, its `noise` and its `decides` entries are made).

Every case of one family sits in ONE handle, as 2K states with the factor (or the interpolation) on (2k, 2k+1), so one wave mixes
straight, stationary, small-angle, near-pi and wrapping intervals.  Each output entry is held to tol = 8 noise + 8 u |exact|, `noise`
being the oracle's own rounding error against its formula in exact arithmetic; no other tolerance appears here.  That a kernel on the
wrong side of a threshold would fail is the `decides` data, asserted without a GPU in tests/test_d3_branch_pins.py."""
import numpy as np
import pytest

import d3_branch_refs as D
import rows_model as RM
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pins():
    return D.load_pins()


def handle(pins, kind, chart, pose, vel, dt):
    import gpslam_amd
    s = gpslam_amd.ChainSolver(kind, chart)
    s.set_qc(np.asarray(pins["Qc"], dtype=float))
    s.set_states(np.asarray(pose, dtype=float), np.asarray(vel, dtype=float))
    s.add_gp_priors(np.arange(0, len(pose), 2), np.full(len(pose) // 2, dt))
    return s


def judge(fam, cases, got_of):
    """every case's device output (flat, in the pin's order) within tol; prints the worst device / tol per branch taken"""
    worst, bad = {}, []
    for k, c in enumerate(cases):
        r = D.ratio(got_of(k), c)
        for fn, b in c["taken"].items():
            worst[fn + ":" + b] = max(worst.get(fn + ":" + b, 0.0), r)
        if not r <= 1.0:
            bad.append((k, c["label"], c["taken"], r))
    print("%s, device / tol by branch: %s" % (fam, {k: float("%.3g" % v) for k, v in sorted(worst.items())}))
    assert not bad, (fam, bad)


@pytest.mark.parametrize("fam", ["gp_prior_pose2", "gp_prior_rot3"])
def test_linearize_gp_within_tol(pins, fam):
    kind, _, chart = D.FAMILIES[fam]
    cases = pins["families"][fam]
    x = [c["inputs"] for c in cases]
    s = handle(pins, kind, chart, [p for c in x for p in (c["p1"], c["p2"])], [v for c in x for v in (c["v1"], c["v2"])], x[0]["dt"])
    assert all(c["dt"] == x[0]["dt"] for c in x)
    s.compile()
    e, H = s.linearize_gp()
    assert e.shape == (len(cases), 6) and H.shape == (len(cases), 4, 6, 3)
    judge(fam, cases, lambda k: np.concatenate([e[k], H[k].ravel()]))
    s.close()


@pytest.mark.parametrize("fam", ["interp_pose2", "interp_rot3"])
def test_interpolate_poses_jac_within_tol(pins, fam):
    kind, _, chart = D.FAMILIES[fam]
    cases = pins["families"][fam]
    x = [c["inputs"] for c in cases]
    s = handle(pins, kind, chart, [p for c in x for p in (c["p1"], c["p2"])], [v for c in x for v in (c["v1"], c["v2"])], x[0]["dt"])
    s.compile()
    left = np.arange(0, 2 * len(cases), 2).astype(np.int32)
    out, H = s.interpolate_poses_jac(left, [c["dt"] for c in x], [c["tau"] for c in x])
    assert H.shape == (len(cases), 4, 3, 3)
    judge(fam, cases, lambda k: np.concatenate([out[k], H[k].ravel()]))
    s.close()


@pytest.mark.parametrize("fam", ["prior_pose2_first_order", "prior_pose2_expmap", "prior_rot3"])
def test_pose_prior_rows_within_tol(pins, fam):
    """unit sigmas: a whitened row of get_rows() is the Jacobian row, rowE the error"""
    kind, _, chart = D.FAMILIES[fam]
    cases = pins["families"][fam]
    x = [c["inputs"] for c in cases]
    K, pd = len(cases), O.POSE_DIM[kind]
    s = handle(pins, kind, chart, [p for c in x for p in (c["x"], c["x"])], np.zeros((2 * K, 3)), 0.5)
    idx = np.arange(0, 2 * K, 2)
    s.add_pose_priors(idx, np.asarray([c["m"] for c in x], dtype=float).reshape(K, pd), np.ones((K, 3)))
    s.compile()
    LR, E, _, _ = s.get_rows()
    rm = RM.row_map(2 * K, 3, gp_left=idx, pri_idx=idx)
    assert LR.shape == (rm.M + rm.Mc, 12)

    def got(k):
        rows = rm.rows_of("pri", k)
        assert not LR[rows, 3:].any()              # a pose prior touches its own pose alone
        return np.concatenate([E[rows], LR[rows, 0:3].ravel()])
    judge(fam, cases, got)
    s.close()


@pytest.mark.parametrize("fam", ["between_pose2_first_order", "between_pose2_expmap", "between_rot3"])
def test_between_rows_within_tol(pins, fam):
    kind, _, chart = D.FAMILIES[fam]
    cases = pins["families"][fam]
    x = [c["inputs"] for c in cases]
    K, pd = len(cases), O.POSE_DIM[kind]
    s = handle(pins, kind, chart, [p for c in x for p in (c["x1"], c["x2"])], np.zeros((2 * K, 3)), 0.5)
    idx = np.arange(0, 2 * K, 2)
    s.add_between(idx, np.asarray([c["m"] for c in x], dtype=float).reshape(K, pd), np.ones((K, 3)))
    s.compile()
    LR, E, _, _ = s.get_rows()
    rm = RM.row_map(2 * K, 3, gp_left=idx, btw_left=idx)
    assert LR.shape == (rm.M + rm.Mc, 12)

    def got(k):
        rows = rm.rows_of("btw", k)
        assert not LR[rows, 3:6].any() and not LR[rows, 9:].any()      # no velocity column
        return np.concatenate([E[rows], LR[rows, 0:3].ravel(), LR[rows, 6:9].ravel()])
    judge(fam, cases, got)
    s.close()


# ---------------------------------------------------------------- the kernel forms of an iteration on the edge chain

def _forms():
    import test_gpu_forms as F
    rec = F.fused(1, b=6, gp=1, lin_rec=1)
    rows = [("records-fused", 0, rec), ("plan-generic-qc", F.PLAN["generic_qc"], rec),
            ("plan-gp-rows", F.PLAN["gp_rows"], F.fused(0, b=6, gp=0, lin_rows=1, lin_rec=0)),
            ("plan-unfused", F.PLAN["unfused"], dict(l0_fused=0, l0_rows=1, l0_column=0, sv=-1, bwd_rows=1)),
            ("plan-column", F.PLAN["column"], dict(l0_fused=0, l0_rows=0, l0_column=1, sv=-1, bwd_rows=0)),
            ("plan-separate-retract", F.PLAN["separate_retract"], rec)]
    return F, rows


MANIFOLDS = [("pose2-first-order", O.POSE2, O.CHART_FIRST_ORDER), ("pose2-expmap", O.POSE2, O.CHART_EXPMAP), ("rot3", O.ROT3, O.CHART_EXPMAP)]
FORM_IDS = ["records-fused", "plan-generic-qc", "plan-gp-rows", "plan-unfused", "plan-column", "plan-separate-retract"]


def _judge(E, kind, what, s1, dev, s0, orc, twin_dist):
    """DESIGN section 2's per-step rule: 1e-9 relative plus ten times the distance between the oracle and its twin"""
    got = E.distance(kind, s1, dev, s0, orc)
    print("%s: device - oracle (error_before, error_after, poses, velocities) %s, twin %s" % (
        what, ["%.2e" % v for v in got], ["%.2e" % v for v in twin_dist]))
    assert (got <= E.REL + E.TWIN * twin_dist).all(), (what, got, twin_dist)


@pytest.mark.parametrize("form", FORM_IDS)
@pytest.mark.parametrize("name,kind,chart", MANIFOLDS, ids=[m[0] for m in MANIFOLDS])
def test_one_iteration_of_every_d3_form_on_the_edge_chain(pins, name, kind, chart, form):
    """tests/d3_edge_chain.py in chunks of 4 (the shapes of tests/test_gpu_forms.py): the census first, then one iterate_gn from the
    oracle's states against the oracle"""
    import gpslam_amd
    import d3_edge_chain as E
    F, rows = _forms()
    _, plan, expect = [r for r in rows if r[0] == form][0]
    feed, _, _ = E.recipe(pins, kind, chart)
    dev = feed(gpslam_amd.ChainSolver(kind, chart, chunk=4, plan=plan))
    info = dev.plan_info()
    dev.launch_census()
    rc1, s1 = dev.iterate_gn()
    F.check_census(dev.launch_census(), expect, name + " " + form, info)          # the form first ...
    orc, s0, twin_dist = E.oracle_and_twin(pins, kind, chart, 1)                   # ... then the numbers
    assert rc1 == 0
    _judge(E, kind, name + " " + form, s1, dev, s0, orc, twin_dist)
    dev.close()


@pytest.mark.parametrize("form,plan,expect", [("folded", 0, dict(lin_pend=1, retract=1, flush=0)), ("separate", 128, dict(lin_pend=0, retract=2, flush=0))],
                         ids=["folded", "separate"])
@pytest.mark.parametrize("name,kind,chart", MANIFOLDS, ids=[m[0] for m in MANIFOLDS])
def test_run_gn_retraction_forms_on_the_edge_chain(pins, name, kind, chart, form, plan, expect):
    """run_gn(2): the first iteration's update applied inside the second K1 (folded) or by k_retract (separate)"""
    import gpslam_amd
    import d3_edge_chain as E
    F, _ = _forms()
    feed, _, _ = E.recipe(pins, kind, chart)
    dev = feed(gpslam_amd.ChainSolver(kind, chart, chunk=4, plan=plan))
    dev.launch_census()
    st, _ = dev.run_gn(2)
    F.check_census(dev.launch_census(), expect, "run_gn(2), %s %s" % (name, form))
    orc, s0, twin_dist = E.oracle_and_twin(pins, kind, chart, 2)
    _judge(E, kind, "run_gn(2), %s %s" % (name, form), st, dev, s0, orc, twin_dist)
    dev.close()
