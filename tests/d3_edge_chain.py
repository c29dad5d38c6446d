"""A 70-state SE(2) / SO(3) chain whose consecutive intervals cycle through the deciding cases of tests/golden/d3_branch_pins.json
(GP prior families) whose tolerance is <= 1e-11: straight and stationary intervals, both sides of every small-angle threshold, a
wrapping angle difference on SE(2).  GP priors, a pose prior on every 20th state (at the state: a residual of exactly zero), a between factor on every interval whose
measurement is the interval's own motion (a residual of rounding size: Log at its first-order branch).  Shared by the CPU test (how far
the oracle's twin lands) and the GPU test (every kernel form an iteration of a d = 3 chain can take)."""
import numpy as np

from oracle import oracle as O

N = 70
REL = 1e-9          # per-step bound of the fp64 path ...
TWIN = 10.0         # ... plus ten times the distance between the oracle and its twin started 1e-15 away
FAMILY = {O.POSE2: "gp_prior_pose2", O.ROT3: "gp_prior_rot3"}


def chain_cases(pins, kind):
    # (SE(2) only: an interval of pi exactly sits on the cut of wrap_pi, not on a threshold -- a start 1e-15 away takes -pi, a different
    # problem, so no twin can say what rounding does to a step there; the pins hold those three cases, the chain leaves them out.  On
    # SO(3) the window's formulas are continuous in R at pi: its four th = pi cases are in the chain.)
    cases = [c for c in pins["families"][FAMILY[kind]]
             if c["tol_max"] <= 1e-11 and max(c["decides"].values(), default=0.0) >= pins["decides_at"]
             and not (kind == O.POSE2 and abs(c["angle"]) == np.pi)]
    assert any(c["angle"] == 0.0 and c["scale"] == 0.0 for c in cases), "no stationary interval"
    if kind == O.POSE2:
        assert any(c["angle"] == 0.0 and c["scale"] > 0.0 for c in cases), "no straight interval"
    return cases


def _step(kind, x, p1, p2):
    """x o (p1^-1 p2), the angle of SE(2) left unwrapped"""
    p1, p2 = np.asarray(p1, dtype=float), np.asarray(p2, dtype=float)
    if kind == O.POSE2:
        c, s = np.cos(p1[2]), np.sin(p1[2])
        h = np.array([c * (p2[0] - p1[0]) + s * (p2[1] - p1[1]), -s * (p2[0] - p1[0]) + c * (p2[1] - p1[1]), p2[2] - p1[2]])
        c, s = np.cos(x[2]), np.sin(x[2])
        return np.array([x[0] + c * h[0] - s * h[1], x[1] + s * h[0] + c * h[1], x[2] + h[2]]), h
    h = p1.reshape(3, 3).T @ p2.reshape(3, 3)
    return (x.reshape(3, 3) @ h).ravel(), h.ravel()


def recipe(pins, kind, chart):
    """(feed, taken): feed(solver) -> the compiled solver; taken: the branches the chain's intervals take, by the pins"""
    cases = chain_cases(pins, kind)
    d, pd = 3, O.POSE_DIM[kind]
    pose, vel, meas = np.zeros((N, pd)), np.zeros((N, d)), np.zeros((N - 1, pd))
    pose[0] = cases[0]["inputs"]["p1"]
    for i in range(N - 1):
        x = cases[i % len(cases)]["inputs"]
        pose[i + 1], meas[i] = _step(kind, pose[i], x["p1"], x["p2"])
        vel[i] = x["v1"]
    vel[N - 1] = cases[(N - 1) % len(cases)]["inputs"]["v1"]
    Qc = np.asarray(pins["Qc"], dtype=float)
    left = np.arange(N - 1).astype(np.int32)
    fix = np.arange(0, N, 20)

    def feed(s, pose0=pose):
        s.set_qc(Qc)
        s.set_states(pose0, vel)
        s.add_gp_priors(left, np.full(N - 1, 0.5))
        s.add_pose_priors(fix, pose[fix], np.full((len(fix), d), 0.01))
        s.add_between(left, meas, np.full((N - 1, d), 0.02))
        s.compile()
        return s
    taken = sorted({fn + ":" + b for c in cases for fn, b in c["taken"].items()})
    return feed, pose, taken


def twin_pose(pose, seed=5):
    return pose * (1.0 + 1e-15 * np.random.default_rng(seed).standard_normal(pose.shape))


def distance(kind, sa, a, sb, b):
    """(error_before, error_after, poses, velocities) of two solvers after the same calls, each relative as tests/test_gpu_forms.py
    judges a step: costs by max(1, cost), poses in local coordinates by max(1, |pose|), velocities by max(1, |vel|)"""
    (xa, va), (xb, vb) = a.get_states(), b.get_states()
    worst = max(float(np.abs(O.local(kind, xa[i], xb[i])).max()) for i in range(len(xa)))
    return np.array([abs(sa.error_before - sb.error_before) / max(1.0, abs(sb.error_before)),
                     abs(sa.error_after - sb.error_after) / max(1.0, abs(sb.error_after)),
                     worst / max(1.0, float(np.abs(xb).max())), float(np.abs(va - vb).max()) / max(1.0, float(np.abs(vb).max()))])


def oracle_and_twin(pins, kind, chart, steps=1):
    """the oracle and its twin (started 1e-15 away) after `steps` Gauss-Newton iterations: (oracle, stats, distance to the twin)"""
    feed, pose, _ = recipe(pins, kind, chart)
    orc, twin = feed(O.Chain(kind, chart)), feed(O.Chain(kind, chart), twin_pose(pose))
    for _ in range(steps):
        (rc0, s0), (rc2, s2) = orc.iterate_gn(), twin.iterate_gn()
        assert rc0 == 0 and rc2 == 0
    return orc, s0, distance(kind, s2, twin, s0, orc)
