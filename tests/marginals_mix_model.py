"""The reference side of the marginals on every factor and noise model: plain numpy plus the oracle.

The reference of every test is np.linalg.inv of a dense H at given states and landmarks: H from O.Chain.normal_equations() on a plain
description of tests/fixed_lag_mix_model.py -- a robust one as reweighted(p, w) with w = np_loss of each factor's own (loss, k) at
the whitened norm of the plain twin's linearize_meas errors --, plus A^T A of state Gaussians (with_state_gaussians), plus the
Lambda of a head prior on the blocks with_state_gaussians / with_border_gaussians touch (state 0; state 0, its landmark coupling
and the landmark block), plus the coupling blocks of loop closures (test_gpu_marginals.oracle_H).

  at                the description at other states (and landmarks)
  oracle            the oracle chain of a plain description
  weights_at        prefix -> (r, w) of a robust description at its own states
  reweighted_at     the plain description a robust one linearises like at its own states, and the weights
  gn                Gauss-Newton steps of the oracle (robust: reweighted at every step's states): the description at the new states
  H_of              the dense H of a plain description, with state Gaussians and head priors
  blocks            (S, S_next, S_lm, S_x_lm) of a dense covariance, the outputs of get_marginals(cross=True)
  worst             the largest distance of such outputs from a dense covariance, in correlation units
  moved             how far the compared blocks of one covariance are from another's, in correlation units
  head_lambda       the Lambda of marginalize_head(k) from the model's recursion on the oracle's arrays
  swap_losses       Huber / Cauchy / Tukey -> Geman-McClure / Welsh / Fair
  closure graphs    the SE(2) / SE(3) loop-closure graphs of the robust closure tests, their losses, norms and weights
"""
import numpy as np

from gpslam_amd import chain as GC
from gpslam_amd import synthetic as S
from oracle import oracle as O
import fixed_lag_mix_model as FM

STEPS = (0, 2)      # marginals at the initial states and after this many Gauss-Newton steps
OTHER = {GC.ROBUST_HUBER: GC.ROBUST_GEMAN_MCCLURE, GC.ROBUST_CAUCHY: GC.ROBUST_WELSH, GC.ROBUST_TUKEY: GC.ROBUST_FAIR}
ROBUST_GRAPHS = ("se2", "se3", "se3_vw", "r3")


def dense_H(D, O_, B=None, HLL=None):
    from test_gpu_marginals import dense_H as f
    return f(D, O_, B, HLL)


def at(p, pose, vel, lm=None):
    q = dict(p, pose=np.array(pose), vel=np.array(vel), N=len(pose))
    if lm is not None and "landmarks" in p:
        q["landmarks"] = np.array(lm)
    return q


def oracle(p):
    return FM.apply(p, FM.chain(p))


# The generator's seed of the robust graphs.  With its default of 7, check_populations cannot hold where the marginals are compared:
# se3_vw's second GPS call has four factors (one Huber, one Cauchy, two Tukey: no loss but Tukey sees both sides of its k at any
# states), and on se2 and r3 every Tukey factor is dead after two Gauss-Newton steps.  Seed 8 is the first at which all four graphs
# pass check_populations at the initial states and after one and two oracle steps; se3 passes with the default and keeps it.
ROBUST_SEED = {"se2": 8, "se3": 7, "se3_vw": 8, "r3": 8}


def graph(name, robust=False, k=5):
    """the graph of the family the marginals tests use: FM.graph at k = 5, SE(2) in the first-order chart"""
    return FM.graph(name, FM.NS[name], k, robust=robust, chart=O.CHART_FIRST_ORDER if name == "se2" else O.CHART_EXPMAP,
                    seed=ROBUST_SEED[name] if robust else 7)


def swap_losses(p):
    q = dict(p)
    for pre in FM.robust_kinds(p):
        q[pre + "_loss"] = np.array([OTHER.get(int(v), int(v)) for v in p[pre + "_loss"]], dtype=np.int32)
    return q


def weights_at(p, errors_from=oracle, scale=1.0):
    """prefix -> (r, w) of the robust description p at its own states; errors_from(plain description) -> a solver with linearize_meas"""
    return FM.robust_weights(p, FM.plain_errors(p, errors_from(FM.plain(p))), scale)


def reweighted_at(p, errors_from=oracle, scale=1.0):
    if not FM.robust_kinds(p):
        return p, {}
    rw = weights_at(p, errors_from, scale)
    return FM.reweighted(p, {pre: w for pre, (r, w) in rw.items()}), rw


def states_of(solver, p):
    pose, vel = solver.get_states()
    return (pose, vel, solver.get_landmarks() if "landmarks" in p else None)


def gn(p, steps):
    """p at the states after `steps` Gauss-Newton steps of the oracle; a robust p is reweighted at every step's own states"""
    for _ in range(steps):
        q, _ = reweighted_at(p)
        orc = oracle(q)
        rc, _ = orc.iterate_gn()
        assert rc == 0
        p = at(p, *states_of(orc, p))
    return p


def add_lambda(H, N, b, Lam, idx=0):
    """H plus a Gaussian's Lambda = A^T A on state idx (b x b: the block with_state_gaussians adds to) or on state idx and all
    landmarks (the blocks with_border_gaussians adds to: D[idx], B[idx], H_LL)"""
    H = H.copy()
    n = Lam.shape[0]
    rows = np.concatenate([np.arange(idx * b, (idx + 1) * b), N * b + np.arange(n - b)])
    assert n == b or N * b + n - b == H.shape[0]
    H[np.ix_(rows, rows)] += Lam
    return H


def H_of(q, gaussians=(), lambdas=()):
    """dense H of the plain description q at its states: the oracle's arrays, A^T A of the state Gaussians (idx, pose_lin, vel_lin, A, c)
    added as FM.with_state_gaussians adds them, and Lambda of (idx, Lambda) added by add_lambda"""
    D, O_, g, B, HLL, _ = oracle(q).normal_equations()
    if gaussians:
        D, g = FM.with_state_gaussians(D, g, q["kind"], q.get("chart", FM.E), q["pose"], q["vel"], gaussians)
    H = dense_H(D, O_, B, HLL)
    for idx, Lam in lambdas:
        H = add_lambda(H, D.shape[0], D.shape[1], Lam, idx)
    return H


def blocks(Sig, N, b):
    """(S, S_next, S_lm, S_x_lm) of the dense covariance Sig, as get_marginals(cross=True) returns them (None without landmarks)"""
    n = N * b
    Sd = np.stack([Sig[i * b:(i + 1) * b, i * b:(i + 1) * b] for i in range(N)])
    Sn = np.stack([Sig[i * b:(i + 1) * b, (i + 1) * b:(i + 2) * b] if i + 1 < N else np.zeros((b, b)) for i in range(N)])
    if Sig.shape[0] == n:
        return Sd, Sn, None, None
    return Sd, Sn, Sig[n:, n:].copy(), Sig[:n, n:].reshape(N, b, -1).copy()


def worst(Sig, out, first=0):
    """largest |out - Sig's blocks| / sqrt(Sig_kk Sig_ll) over S, S_next (but the last, which must be exactly zero), S_lm, S_x_lm;
    out holds the states first .. of Sig"""
    Sd, Sn = out[0], out[1]
    Slm, Sxl = (out[2], out[3]) if len(out) == 4 else (None, None)
    count, b = Sd.shape[0], Sd.shape[1]
    dg = np.sqrt(np.diag(Sig))
    nall = Sig.shape[0] - (Slm.shape[0] if Slm is not None else 0)
    N = nall // b
    assert first + count == N and N * b == nall
    w = 0.0
    for i in range(count):
        r = slice((first + i) * b, (first + i + 1) * b)
        w = max(w, float(np.max(np.abs(Sd[i] - Sig[r, r]) / np.outer(dg[r], dg[r]))))
        if i + 1 < count:
            r2 = slice((first + i + 1) * b, (first + i + 2) * b)
            w = max(w, float(np.max(np.abs(Sn[i] - Sig[r, r2]) / np.outer(dg[r], dg[r2]))))
        if Sxl is not None:
            w = max(w, float(np.max(np.abs(Sxl[i] - Sig[r, nall:]) / np.outer(dg[r], dg[nall:]))))
    assert np.all(Sn[count - 1] == 0.0), "the last Sigma_{i,i+1} is not exactly zero"
    if Slm is not None:
        w = max(w, float(np.max(np.abs(Slm - Sig[nall:, nall:]) / np.outer(dg[nall:], dg[nall:]))))
    return w


def moved(Sig, other, N, b):
    """how far the compared blocks of the dense covariance `other` are from Sig's, in Sig's correlation units"""
    return worst(Sig, blocks(other, N, b))


def head_lambda(p, k, onto):
    """Lambda of the head of the plain description p, by the model's recursion on the oracle's arrays: b x b, or over (state, landmarks)"""
    return FM.head_reference(p, k, onto)[0]


# (name, k, onto, robust): marginalize_head(k) leaves the covariance of the remaining states and the landmarks as it was
SCHUR = ([(n, k, False, False) for n in ("se3_vw", "so3") for k in (1, 5, FM.NS[n] - 1)]
         + [(n, k, onto, False) for n in ("se2", "r3") for k in (1, 5, FM.NS[n] - 1) for onto in (True, False)]
         + [("se3", k, True, True) for k in (1, 5, FM.NS["se3"] - 1)])


def schur_case(name, k, onto, robust):
    return FM.case(name, k, onto, robust=robust, chart=O.CHART_FIRST_ORDER if name == "se2" else O.CHART_EXPMAP)


def direct_gaussians(p, seed=3):
    """state Gaussians (idx, pose_lin, vel_lin, A, c) on state 3 and on the last state: random full-rank A, linearised a few tenths
    away from the current state (the draw of tests/test_gpu_fixed_lag_mix.py's inner_gaussians)"""
    rng = np.random.default_rng(seed)
    kind, d = p["kind"], O.TANGENT_DIM[p["kind"]]
    out = []
    for i in (3, p["pose"].shape[0] - 1):
        pl = O.retract(kind, p["pose"][i], 0.3 * rng.standard_normal(d), p.get("chart", FM.E))
        vl = p["vel"][i] + 0.3 * rng.standard_normal(d)
        out.append((i, pl, vl, 20.0 * rng.standard_normal((2 * d, 2 * d)), 20.0 * rng.standard_normal(2 * d)))
    return out


# ---------------------------------------------------------------------------------------------------------------- loop closures
CLOSURE_LOSS = [GC.ROBUST_HUBER, GC.ROBUST_CAUCHY, GC.ROBUST_TUKEY]
CLOSURE_STEPS = 2       # Gauss-Newton steps before the closure graphs' marginals
SEGMENTED_STEPS = 2     # ... and before the segmented case's
SEGMENTED_K = (0.3, 0.5)


def check_closure_populations(p, r, w):
    """closure 2 (Tukey) is dead, closure 0 (Huber) is beyond its k, another Huber closure within it, none within 1e-6 of a kink"""
    loss, k = p["closure_loss"], p["closure_k"]
    assert loss[2] == GC.ROBUST_TUKEY and w[2] == 0.0
    assert loss[0] == GC.ROBUST_HUBER and 0.0 < w[0] < 1.0
    assert ((loss == GC.ROBUST_HUBER) & (w == 1.0)).any()
    kinked = (loss == GC.ROBUST_HUBER) | (loss == GC.ROBUST_TUKEY)
    assert np.all(np.abs(r[kinked] - k[kinked]) > 1e-6 * k[kinked])


def closure_graph(name):
    """(description with closure_loss / closure_k, chart, passes or None): the robust loop-closure graphs.
      pose2_5      SE(2), 60 states, 5 closures in one pass
      pose2_5_lm   the same beside 6 landmarks: R = 1 + 6 * 2 + 5 * 3 = 28 (test_gpu_marginals.test_closures_against_the_oracle)
      pose2_12     SE(2), 60 states, 12 closures in two column passes (9 + 3)
      pose3_6      SE(3), 60 states, 6 closures in two column passes (4 + 2)
    Losses Huber, Cauchy, Tukey in turn with k = 3, 3.3, 3.6, ...; closure 0 (Huber) is displaced by 0.15 m (7.5 sigma: w < 1),
    closure 2 (Tukey) by 2 m (w = 0), closure 4 (Cauchy) by 0.1 m."""
    from test_gpu_closure import _anchored, _strip_landmarks
    from test_gpu_closure_passes import _pairs as closure_pairs
    if name in ("pose2_5", "pose2_5_lm"):
        p = _anchored(S.pose2_range_chain(60, L=6, seed=1))
        if name == "pose2_5":
            p = _strip_landmarks(p)
        p = S.add_loop_closures(p, [[2, 40], [5, 50], [10, 58], [20, 45], [0, 30]], seed=5)
        passes = None
    elif name == "pose2_12":
        p = S.add_loop_closures(_anchored(_strip_landmarks(S.pose2_range_chain(60, seed=9))), closure_pairs(60, 12, 21), seed=5)
        passes = (12, 9, 2)
    elif name == "pose3_6":
        p = S.add_loop_closures(S.pose3_chain(60, seed=2), closure_pairs(60, 6, 31), seed=8)
        passes = (6, 4, 2)
    else:
        raise ValueError(name)
    K = len(p["closure_first"])
    m = p["closure_meas"].copy()
    col = 9 if p["kind"] == O.POSE3 else 0
    m[0, col] += 0.15
    m[2, col] += 2.0
    m[4, col + 1] -= 0.1
    p["closure_meas"] = m
    p["closure_loss"] = np.array([CLOSURE_LOSS[f % 3] for f in range(K)], dtype=np.int32)
    p["closure_k"] = 3.0 + 0.3 * np.arange(K)
    return p, O.CHART_EXPMAP, passes


def closure_weights(p, pose, chart, scale=1.0):
    """(r, w) of the closures of p at the poses `pose`: r from the oracle's BetweenFactor error (test_gpu_robust._closure_norms)"""
    from test_gpu_robust import _closure_norms, np_loss
    r = _closure_norms(p, pose, chart)
    w = np.array([float(np_loss(FM.LOSS_NAMES[int(l)], float(k), v)[0]) * scale for l, k, v in zip(p["closure_loss"], p["closure_k"], r)])
    return r, w


def closure_reweighted(p, w):
    """the plain description whose closure sigmas are sigma / sqrt(w); a closure with w = 0 is dropped"""
    q = {key: v for key, v in p.items() if key not in ("closure_loss", "closure_k")}
    keep = w > 0.0
    for key in ("closure_first", "closure_second", "closure_meas"):
        q[key] = np.asarray(p[key])[keep]
    q["closure_sig"] = np.asarray(p["closure_sig"])[keep] / np.sqrt(w[keep])[:, None]
    return q


def closure_oracle(q, chart):
    return S.apply(q, O.Chain(q["kind"], chart, 2 if "landmarks" in q else 0))


class _States:
    """what test_gpu_marginals.oracle_H asks of a device handle, from arrays"""

    def __init__(self, q, pose, vel, lm):
        self.pose, self.vel, self.lm = pose, vel, lm
        self.L = 0 if lm is None else len(lm)
        self.d = O.TANGENT_DIM[q["kind"]]
        self.b, self.pd = 2 * self.d, O.POSE_DIM[q["kind"]]

    def get_states(self):
        return self.pose, self.vel

    def get_landmarks(self):
        return self.lm


def closure_H(q, chart, pose, vel, lm=None):
    """dense H of the plain closure description q at (pose, vel, lm), coupling blocks as test_gpu_marginals.oracle_H adds them"""
    from test_gpu_marginals import oracle_H
    return oracle_H(closure_oracle(q, chart), _States(q, pose, vel, lm), q)


def closure_gn(p, chart, steps):
    """(pose, vel, lm) after `steps` oracle Gauss-Newton steps of the robust closure description, reweighted at every step's states"""
    pose, vel, lm = p["pose"], p["vel"], p.get("landmarks")
    for _ in range(steps):
        r, w = closure_weights(p, pose, chart)
        q = dict(closure_reweighted(p, w), pose=pose, vel=vel)
        if lm is not None:
            q["landmarks"] = lm
        orc = closure_oracle(q, chart)
        rc, _ = orc.iterate_gn()
        assert rc == 0
        pose, vel = orc.get_states()
        lm = orc.get_landmarks() if lm is not None else None
    return pose, vel, lm


# ---------------------------------------------------------------------------------------------------------------- the segmented case
def segmented_graph():
    """_anchored_range_chain(60) of tests/test_gpu_marginals.py (8 landmarks; segment_length 30: cuts at 0, 30 and 59, two segments,
    the smallest graph of tests/test_gpu_marginals_segmented.py with an inner cut) in the FM description's keys, with a Huber and a
    Cauchy loss in turn on its interpolated ranges.  Its 31 ranges leave whitened residuals of 0.03 .. 0.65 behind two Gauss-Newton
    steps, so k = 0.3 (Huber) and 0.5 (Cauchy) put residuals on both sides."""
    from test_gpu_marginals import _anchored_range_chain
    p = _anchored_range_chain(60)
    M = len(p["range_left"])
    q = {key: p[key] for key in ("kind", "qc", "N", "pose", "vel", "gp_left", "gp_dt", "prior_idx", "prior_pose", "prior_sig", "between_left",
                                 "between_meas", "between_sig", "landmarks", "lprior_idx", "lprior", "lprior_sig", "range_left", "range_lm",
                                 "range_sigma", "range_dt", "range_tau")}
    q.update(chart=O.CHART_EXPMAP, ld=2, range_z=p["range_z"], range_call=np.ones(M, dtype=np.int32),
             range_loss=np.where(np.arange(M) % 2 == 0, GC.ROBUST_HUBER, GC.ROBUST_CAUCHY).astype(np.int32),
             range_k=np.where(np.arange(M) % 2 == 0, SEGMENTED_K[0], SEGMENTED_K[1]))
    return q
