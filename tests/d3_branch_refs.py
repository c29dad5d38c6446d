"""What the tests of tests/golden/d3_branch_pins.json share with its generator (tests/golden/make_d3_branch_pins.py): the families,
the oracle's evaluation of one case, the tolerance and the conditions on the `decides` data.  No mpmath here."""
import json
import os

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53

FAMILIES = {  # name: (kind, what, chart)
    "gp_prior_pose2": (O.POSE2, "gp", O.CHART_EXPMAP), "gp_prior_rot3": (O.ROT3, "gp", O.CHART_EXPMAP),
    "interp_pose2": (O.POSE2, "interp", O.CHART_EXPMAP), "interp_rot3": (O.ROT3, "interp", O.CHART_EXPMAP),
    "prior_pose2_first_order": (O.POSE2, "prior", O.CHART_FIRST_ORDER), "prior_pose2_expmap": (O.POSE2, "prior", O.CHART_EXPMAP),
    "between_pose2_first_order": (O.POSE2, "between", O.CHART_FIRST_ORDER), "between_pose2_expmap": (O.POSE2, "between", O.CHART_EXPMAP),
    "prior_rot3": (O.ROT3, "prior", O.CHART_EXPMAP), "between_rot3": (O.ROT3, "between", O.CHART_EXPMAP),
}
# functions whose branch variable is the blended xi of an interpolation, not the relative motion
EXP_SIDE = ("se2_exp", "se2_dexp", "so3_exp", "so3_jr")


def load_pins():
    with open(os.path.join(HERE, "golden", "d3_branch_pins.json")) as f:
        return json.load(f)


def oracle_eval(fam, x, Qc):
    """the oracle's [e | H] of one case's inputs, flat, in the order of the pins"""
    kind, what, chart = FAMILIES[fam]
    if what == "gp":
        e, H = O.gp_prior(kind, x["p1"], x["v1"], x["p2"], x["v2"], x["dt"])
        return np.concatenate([e] + [h.ravel() for h in H])
    if what == "interp":
        Lam, Psi = O.lambda_psi(3, np.asarray(Qc, dtype=float), x["dt"], x["tau"])
        out, H = O.interpolate(kind, Lam, Psi, x["p1"], x["v1"], x["p2"], x["v2"])
        return np.concatenate([out] + [h.ravel() for h in H])
    e = np.zeros(3)
    if what == "prior":
        H = np.zeros(9)
        O.call("orc_prior_factor", kind, chart, O.A(x["m"]), O.A(x["x"]), e, H)
        return np.concatenate([e, H])
    H1, H2 = np.zeros(9), np.zeros(9)
    O.call("orc_between_factor", kind, chart, O.A(x["m"]), O.A(x["x1"]), O.A(x["x2"]), e, H1, H2)
    return np.concatenate([e, H1, H2])


def pin_of(case):
    return np.asarray(case["e"] + case["H"], dtype=float)


def tol_of(case):
    """8 noise + 8 u |exact|, entry by entry"""
    return 8.0 * np.asarray(case["noise"], dtype=float) + 8.0 * U * np.abs(pin_of(case))


def ratio(got, case):
    """largest |got - pin| / tol over the entries of a case (an entry whose pin and noise are both zero must be met exactly)"""
    d, t = np.abs(np.asarray(got, dtype=float).ravel() - pin_of(case)), tol_of(case)
    if (d[t == 0] != 0).any() or not np.isfinite(d).all():
        return np.inf
    return float((d[t > 0] / t[t > 0]).max()) if (t > 0).any() else 0.0


def branch_variable(fn, case):
    """the grid angle that steers `fn` in a case: the blended xi's for the Exp side of an interpolation, else that of the relative motion"""
    return case.get("xi_angle", case["angle"]) if fn in EXP_SIDE else case["angle"]


def conditions(fams, named, decides_at):
    """the table of (function, branch, side) from the cases' `decides` entries: (table, undecidable, problems).  A side that any case
    decides must have a deciding case in every family that reaches it; every named branch must be taken somewhere."""
    sides = {}
    for fam, cases in fams.items():
        for c in cases:
            for key, r in c["decides"].items():
                sd = sides.setdefault(key, dict(families={}, noise=0.0, best=0.0, at={}))
                sd["families"].setdefault(fam, []).append(r)
                sd["noise"] = max(sd["noise"], max(c["noise"]))
                sd["best"] = max(sd["best"], r)
                at = branch_variable(key.split(":")[0], c)
                sd["at"][at] = max(sd["at"].get(at, 0.0), r)
    table, undecidable, problems = [], [], []
    for key in sorted(sides):
        sd = sides[key]
        decided = sd["best"] >= decides_at
        missing = [f for f, r in sd["families"].items() if max(r) < decides_at] if decided else []
        if missing:
            problems.append("%s is decidable but has no deciding case in %s" % (key, missing))
        if not decided:
            undecidable.append(key)
        fn, rest = key.split(":")
        table.append(dict(function=fn, branch=rest.split("|")[0], side=rest.split("|")[1], largest_noise=sd["noise"],
                          best_ratio=sd["best"], deciding_cases=sum(r >= decides_at for rs in sd["families"].values() for r in rs),
                          decided=decided, value_check_only_at=sorted(a for a, r in sd["at"].items() if r < decides_at)))
    taken = {(fn, b) for cases in fams.values() for c in cases for fn, b in c["taken"].items()}
    for nb in named:
        if tuple(nb) not in taken:
            problems.append("branch %s:%s is never taken" % tuple(nb))
    return table, undecidable, problems
