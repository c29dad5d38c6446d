"""Robust noise models (noiseModel::Robust over an mEstimator) on measurement factors and loop closures, on the HIP path.

The oracle has no robust model, so the yardstick is an identity the plain product can evaluate: a robust handle at given states
linearises exactly like a plain handle of the same graph whose sigmas are sigma / sqrt(w) (or whose covariance is cov / w), with
the weights w computed here in numpy from the plain handle's own gpslam_hip_linearize_meas errors.

Every graph has 70 states (two level-0 chunk boundaries) and 131 measurement factors of the kind under test (one thread block of
128, a ragged second one, a factor on the last interval / state); measurements are seeded and about one factor in ten is displaced
by 30-80 sigma.  The plain side of a graph (measurements, residual norms, rows, cost) is computed once per graph and shared by
the six losses."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from gpslam_amd import synthetic as S
from test_gpu_parity import gpu, random_chain, states_close

pytestmark = pytest.mark.gpu

N, M, L = 70, 131, 4
LOSSES = ["HUBER", "CAUCHY", "TUKEY", "GEMAN_MCCLURE", "WELSH", "FAIR"]
# case -> (manifold, landmark dim, MEAS_* kind, rows, sigma per row)
CASES = {
    "interp-range-pose2": (O.POSE2, 2, 0, 1, [0.05]),
    "interp-range-pose3": (O.POSE3, 3, 0, 1, [0.05]),
    "range-linear3": (O.LINEAR3, 2, 1, 1, [0.05]),
    "bearing-range-linear3": (O.LINEAR3, 2, 5, 2, [0.02, 0.05]),
    "odometry2d-linear3": (O.LINEAR3, 0, 4, 3, [0.02, 0.02, 0.01]),
    "interp-attitude-rot3": (O.ROT3, 0, 2, 2, [0.01, 0.01]),      # (|e| <= 1: 80 sigma must fit)
    "interp-gps-pose3": (O.POSE3, 0, 3, 3, [0.05, 0.04, 0.06]),
    "interp-gps-pose3-cov": (O.POSE3, 0, 3, 3, [0.05, 0.04, 0.06]),
    "interp-projection-pose3": (O.POSE3, 3, 6, 2, [1.0, 1.5]),
}
K_CAL = np.array([500.0, 480.0, 0.5, 320.0, 240.0])


def np_loss(loss, k, r):
    """(w, rho) of the issue's table, plain numpy on arrays"""
    r = np.asarray(r, dtype=np.float64)
    u = r * r / (k * k)
    with np.errstate(divide="ignore", invalid="ignore"):
        if loss == "HUBER":
            return np.where(r <= k, 1.0, k / np.maximum(r, 1e-300)), np.where(r <= k, 0.5 * r * r, k * (r - 0.5 * k))
        if loss == "CAUCHY":
            return 1.0 / (1.0 + u), 0.5 * k * k * np.log1p(u)
        if loss == "TUKEY":
            return np.where(r <= k, (1.0 - u) ** 2, 0.0), np.where(r <= k, k * k * (1.0 - (1.0 - u) ** 3) / 6.0, k * k / 6.0)
        if loss == "GEMAN_MCCLURE":
            return 1.0 / (1.0 + u) ** 2, 0.5 * r * r / (1.0 + u)
        if loss == "WELSH":
            return np.exp(-u), -0.5 * k * k * np.expm1(-u)
        if loss == "FAIR":
            return 1.0 / (1.0 + r / k), k * k * (r / k - np.log1p(r / k))
    raise ValueError(loss)


def loss_id(loss):
    return getattr(gpu().chain, "ROBUST_" + loss)


class Graph:
    """One seeded graph: base chain + 131 factors of one kind.  feed(solver, sig=..., cov=..., loss=...) builds it."""

    def __init__(self, case, seed=5):
        self.case = case
        self.kind, self.ld, self.mk, self.rows, sig = CASES[case]
        self.d = O.TANGENT_DIM[self.kind]
        self.chart = O.CHART_FIRST_ORDER if self.kind == O.POSE2 else O.CHART_EXPMAP
        rng = np.random.default_rng(1000 + seed)
        self.c = random_chain(self.kind, N, seed, motion=0.3, noise=0.02)
        self.Qc = np.diag(0.01 + 0.02 * rng.random(self.d))
        self.sig = np.tile(np.array(sig), (M, 1))
        self.full_cov = case.endswith("-cov")
        if self.full_cov:      # a full SPD covariance per factor with the sigmas above on its diagonal
            Cm = np.array([[1.0, 0.3, -0.2], [0.3, 1.0, 0.25], [-0.2, 0.25, 1.0]])
            self.cov = np.array([np.outer(s, s) * Cm for s in self.sig])
        self.single = self.mk in (1, 5)                       # one-state kinds
        idx = np.sort(rng.integers(0, N if self.single else N - 1, size=M)).astype(np.int32)
        idx[-1] = N - 1 if self.single else N - 2             # a factor on the last state / interval
        self.idx = idx
        self.dt = self.c["dt"][np.minimum(idx, N - 2)]
        self.tau = self.dt * rng.uniform(0.05, 0.95, M)
        self.lm = rng.integers(0, L, size=M).astype(np.int32) if self.ld else None
        if self.ld == 3 and self.mk == 6:
            # four landmarks 30 m out in tetrahedral directions; every factor looks at the one nearest its camera axis (body z), so that
            # whichever way the random trajectory turns the point is in front of the camera, at most 55 degrees off the axis
            tp = self.c["truth_pose"]
            self.lands = tp[:, 9:12].mean(0) + 30.0 / np.sqrt(3.0) * np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
            zc = np.einsum("nj,nlj->nl", tp[idx, :9].reshape(-1, 3, 3)[:, :, 2], self.lands[None] - tp[idx, None, 9:12])
            self.lm = np.argmax(zc, axis=1).astype(np.int32)
        elif self.ld:
            self.lands = rng.uniform(-6, 6, (L, self.ld)) + (self.c["truth_pose"][0, 9:12] if self.kind == O.POSE3 else 0.0)
        else:
            self.lands = None
        self.meas = None
        self.nz = self.bref = None
        if self.mk == 2:                                      # attitude: nZ fixed, bRef = R(tau)^T nZ + noise (tests/test_gpu_measurements.py)
            from test_gpu_measurements import interp_truth
            self.nz = np.tile([0.0, 0.0, 1.0], (M, 1))
            bref = []
            for i, t in zip(idx, self.tau):
                R = interp_truth(self.kind, self.Qc, self.c, int(i), float(t)).reshape(3, 3)
                bref.append(R.T @ np.array([0.0, 0.0, 1.0]))
            b0 = np.array(bref)
            perp = np.cross(b0, [1.0, 0.0, 0.0])
            perp /= np.linalg.norm(perp, axis=1, keepdims=True)
            out = rng.random(M) < 0.1
            out[:2] = [True, False]
            th = np.arcsin(rng.uniform(30, 80, M) * self.sig[0, 0])      # displaced by 30-80 sigma in the tangent plane
            b0 = np.where(out[:, None], np.cos(th)[:, None] * b0 + np.sin(th)[:, None] * perp, b0)
            bref = b0 + self.sig[0, 0] * rng.standard_normal((M, 3))
            self.bref = bref
        else:                                                 # prediction h(x_truth) from the device itself: e(z = 0) at the truth
            zero = np.zeros((M, self.rows))
            tmp = self._build(gpu().ChainSolver(self.kind, self.chart, self.ld), zero, states=(self.c["truth_pose"], self.c["truth_vel"]))
            pred, _ = tmp.linearize_meas(self.mk, M)
            tmp.close()
            noise = self.sig * rng.standard_normal((M, self.rows))
            out = rng.random(M) < 0.1
            out[:2] = [True, False]                           # (both populations exist whatever the draw)
            disp = rng.uniform(30, 80, (M, self.rows)) * self.sig * np.where(rng.random((M, self.rows)) < 0.5, -1.0, 1.0)
            self.meas = pred + noise + np.where(out[:, None], disp, 0.0)
        self.outlier = out

    def _add(self, s, meas, sig, cov):
        i, mk = self.idx, self.mk
        if mk == 0:
            s.add_interp_range(i, self.lm, meas[:, 0], sig[:, 0], self.dt, self.tau)
        elif mk == 1:
            s.add_range(i, self.lm, meas[:, 0], sig[:, 0])
        elif mk == 2:
            s.add_interp_attitude(i, self.nz, self.bref, sig, self.dt, self.tau)
        elif mk == 3 and cov is None:
            s.add_interp_gps(i, meas, sig, self.dt, self.tau)
        elif mk == 3:
            # one call per run of factors with / without a finite covariance (w = 0 of a redescending loss: infinite sigmas instead)
            fin = np.isfinite(cov).all(axis=(1, 2))
            a = 0
            while a < M:
                b = a
                while b < M and fin[b] == fin[a]:
                    b += 1
                s.add_interp_gps(i[a:b], meas[a:b], sig[a:b] if fin[a] else np.full((b - a, 3), np.inf), self.dt[a:b], self.tau[a:b])
                if fin[a]:
                    s.set_meas_covariance(3, cov[a:b])
                a = b
        elif mk == 4:
            s.add_odometry2d(i, meas, sig)
        elif mk == 5:
            s.add_bearing_range(i, self.lm, meas[:, 0], meas[:, 1], sig)
        elif mk == 6:
            s.add_interp_projection(i, self.lm, meas, sig, self.dt, self.tau, K_CAL)

    def _build(self, s, meas, sig=None, cov=None, loss=None, k=None, states=None):
        c, d = self.c, self.d
        s.set_qc(self.Qc)
        s.set_states(*(states if states is not None else (c["pose"], c["vel"])))
        if self.ld:
            s.set_landmarks(self.lands + 0.05)
        s.add_gp_priors(np.arange(N - 1), c["dt"])
        fix = np.arange(0, N, 16)
        s.add_pose_priors(fix, c["truth_pose"][fix], np.full((len(fix), d), 0.02))
        if self.mk != 3:                                      # (interpolated GPS: no velocity priors, so that the plain graph takes the line form)
            s.add_vel_priors([0, N - 1], c["truth_vel"][[0, N - 1]], np.full((2, d), 0.05))
        if self.ld:
            s.add_landmark_priors(np.arange(L), self.lands, np.full((L, self.ld), 0.5))
        self._add(s, meas, self.sig if sig is None else sig, cov)
        if loss is not None:
            s.set_meas_robust(self.mk, np.full(M, loss, dtype=np.int32), np.full(M, k))
        s.compile()
        return s

    def feed(self, sig=None, cov=None, loss=None, k=None, **kw):
        cov = cov if cov is not None else (self.cov if self.full_cov else None)
        return self._build(gpu().ChainSolver(self.kind, self.chart, self.ld, **kw), self.meas, sig=sig, cov=cov, loss=loss, k=k)

    def rnorm(self, e):
        """|whitened error|_2 per factor from unwhitened errors (M x rows)"""
        if self.full_cov:
            return np.sqrt(np.einsum("fi,fij,fj->f", e, np.linalg.inv(self.cov), e))
        return np.sqrt(np.sum((e / self.sig) ** 2, axis=1))

    def reweighted(self, w, **kw):
        """the plain handle whose sigmas are sigma / sqrt(w) (covariance: cov / w)"""
        with np.errstate(divide="ignore"):
            if self.full_cov:
                return self.feed(cov=self.cov / w[:, None, None], **kw)
            return self.feed(sig=self.sig / np.sqrt(w)[:, None], **kw)


@functools.lru_cache(maxsize=None)
def plain_side(case):
    """(graph, residual norms r, plain cost, k) of a case, computed once"""
    g = Graph(case)
    h = g.feed()
    e, _ = h.linearize_meas(g.mk, M)
    r = g.rnorm(e)
    err = h.error()
    h.close()
    k = float(np.sqrt(np.median(r) * r.max()))        # between the bulk and the displaced factors
    return g, r, err, k


def rows_of(h):
    LR, E, Mm, Lm = h.get_rows()
    return np.concatenate([LR, E[:, None]] + ([Mm] if Mm is not None else []), axis=1)


def check_identity(g, r, err_plain, k, loss, rows=True, **kw):
    """the reweighting identity of one graph and one loss: rows, cost, one Gauss-Newton step, weights"""
    w, rho = np_loss(loss, k, r)
    assert (r < k).any() and (r > k).any(), (r.min(), k, r.max())
    rob = g.feed(loss=loss_id(loss), k=k, **kw)
    ref = g.reweighted(w, **kw)
    out = {}
    if rows:
        A, B = rows_of(rob), rows_of(ref)
        assert A.shape == B.shape
        scale = np.abs(B).max(axis=1)
        out["rows"] = float((np.abs(A - B).max(axis=1) / np.maximum(scale, 1e-300))[scale > 0].max())
        zero_rows = np.abs(A[scale == 0]).max() if (scale == 0).any() else 0.0
    want = float(np.sum(rho)) + (err_plain - 0.5 * float(np.sum(r * r)))
    got = rob.error()
    out["error"] = abs(got - want) / want
    wd = rob.meas_weights(g.mk, M)
    out["weights"] = float(np.abs(wd - w).max())
    rc0, s0 = rob.iterate_gn()
    rc1, s1 = ref.iterate_gn()
    assert rc0 == 0 and rc1 == 0
    print("%s %s k=%.3f: %s |delta| %.3e / %.3e, below k %d above k %d" % (g.case, loss, k, out, s0.delta_inf_norm, s1.delta_inf_norm, (r < k).sum(), (r > k).sum()))
    if rows:
        assert zero_rows == 0.0
        assert out["rows"] <= 1e-11, out
    assert out["error"] <= 1e-12, (out, got, want)
    assert out["weights"] <= 1e-13, out
    assert abs(s0.error_before - got) <= 1e-12 * got
    states_close(g.kind, *ref.get_states(), *rob.get_states(), 1e-9)
    if g.ld:
        l0, l1 = ref.get_landmarks(), rob.get_landmarks()
        assert np.abs(l0 - l1).max() <= 1e-9 * max(1.0, np.abs(l0).max())
    rob.close()
    ref.close()


# ---------------------------------------------------------------- 1. the reweighting identity
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", list(CASES))
def test_reweighting_identity(case, loss):
    g, r, err, k = plain_side(case)
    assert 5 <= g.outlier.sum() <= 30
    check_identity(g, r, err, k, loss)


# ---------------------------------------------------------------- 2. no loss, no change
@pytest.mark.parametrize("how", ["NONE", "HUBER-1e300"])
def test_no_op_losses_change_nothing(how):
    g, r, err, k = plain_side("interp-range-pose2")
    gp = gpu()
    a = g.feed()
    b = g.feed(loss=gp.chain.ROBUST_NONE, k=1.0) if how == "NONE" else g.feed(loss=gp.chain.ROBUST_HUBER, k=1e300)
    assert a.plan_info() == b.plan_info()
    for _ in range(3):
        a.iterate_gn()
        b.iterate_gn()
    (xa, va), (xb, vb) = a.get_states(), b.get_states()
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert np.array_equal(a.get_landmarks(), b.get_landmarks())
    assert np.array_equal(b.meas_weights(g.mk, M), np.ones(M))


# ---------------------------------------------------------------- 3. loop closures
def _closure_graph(kind):
    if kind == O.POSE2:
        p = S.pose2_range_chain(N, L=4, seed=3)
        p = {k: v for k, v in p.items() if not (k.startswith("range_") or k.startswith("lprior") or k.startswith("landmark"))}
        p["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
    else:
        p = S.pose3_chain(N, seed=2)
        p["truth"] = p["pose"].copy()
    p = S.add_loop_closures(p, [[3, 60], [66, 20], [10, 45]], seed=5)
    m = p["closure_meas"].copy()
    m[1, 0 if kind == O.POSE2 else 9] += 2.0                  # the second closure is false: its measured pose is 2 m off
    p["closure_meas"] = m
    return p


def _closure_norms(p, pose, chart):
    """r of every closure from the oracle's BetweenFactor error: a three-state oracle chain that holds nothing but the closure"""
    kind, d = p["kind"], O.TANGENT_DIM[p["kind"]]
    r = []
    for a, b, m, sg in zip(p["closure_first"], p["closure_second"], p["closure_meas"], p["closure_sig"]):
        o = O.Chain(kind, chart)
        o.set_qc(np.eye(d))
        o.set_states(np.stack([pose[a], pose[a], pose[b]]), np.zeros((3, d)))
        o.add_between_pairs([0], [2], m[None], sg[None])
        o.compile()
        r.append(np.sqrt(2.0 * o.error()))
    return np.array(r)


def _check_closures(p, loss, ld=0, chart=O.CHART_EXPMAP):
    gp = gpu()
    K = len(p["closure_first"])
    plain = S.apply(p, gp.ChainSolver(p["kind"], chart, ld))
    r = _closure_norms(p, p["pose"], chart)
    k = float(np.sqrt(np.median(r) * r.max()))
    assert (r < k).any() and (r > k).any(), (r, k)
    w, rho = np_loss(loss, k, r)
    want = float(np.sum(rho)) + (plain.error() - 0.5 * float(np.sum(r * r)))

    def robust(s):
        s.set_between_pairs_robust(np.full(K, loss_id(loss), dtype=np.int32), np.full(K, k))
        s.compile()
        return s
    q = dict(p)
    with np.errstate(divide="ignore"):
        q["closure_sig"] = p["closure_sig"] / np.sqrt(w)[:, None]
    rob = robust(S.apply(p, gp.ChainSolver(p["kind"], chart, ld)))
    ref = S.apply(q, gp.ChainSolver(p["kind"], chart, ld))
    got = rob.error()
    wd = rob.between_pairs_weights(K)
    rc0, s0 = rob.iterate_gn()
    rc1, s1 = ref.iterate_gn()
    print("closures %s %s: r %s k %.3f w %s / %s error %.12g / %.12g |delta| %.3e / %.3e" % (p["kind"], loss, r, k, wd, w, got, want, s0.delta_inf_norm, s1.delta_inf_norm))
    assert rc0 == 0 and rc1 == 0
    assert np.abs(wd - w).max() <= 1e-13
    assert abs(got - want) <= 1e-12 * want
    assert abs(s0.error_before - got) <= 1e-12 * got
    states_close(p["kind"], *ref.get_states(), *rob.get_states(), 1e-9)
    if ld:
        l0, l1 = ref.get_landmarks(), rob.get_landmarks()
        assert np.abs(l0 - l1).max() <= 1e-9 * max(1.0, np.abs(l0).max())
    for s in (plain, rob, ref):
        s.close()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kind", [O.POSE2, O.POSE3], ids=["pose2", "pose3"])
def test_closures_reweighting_identity(kind, loss):
    _check_closures(_closure_graph(kind), loss)


@pytest.mark.parametrize("loss", ["HUBER", "TUKEY"])
def test_closures_beside_landmarks(loss):
    """the SE(2) graph of tests/test_gpu_closure.py's shape: interpolated ranges to 4 landmarks and closures share the border"""
    p = S.pose2_range_chain(N, L=4, seed=3)
    p["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
    p = S.add_loop_closures(p, [[3, 60], [66, 20]], seed=7)
    m = p["closure_meas"].copy()
    m[1, 0] += 2.0
    p["closure_meas"] = m
    _check_closures(p, loss, ld=2, chart=O.CHART_FIRST_ORDER)


# ---------------------------------------------------------------- 4. it converges and it helps
def _plaza(outliers=True):
    """Plaza-shaped: SE(2), 70 states, 4 landmarks with priors, 131 interpolated ranges at sigma 0.5, 13 of them 5 m long"""
    p = S.pose2_range_chain(N, L=4, seed=11)
    rng = np.random.default_rng(4242)
    left = np.sort(rng.integers(0, N - 1, size=M)).astype(np.int32)
    left[-1] = N - 2
    dt = 0.1
    tau = dt * rng.uniform(0.05, 0.95, M)
    lm = rng.integers(0, 4, size=M).astype(np.int32)
    t = p["truth"]
    at = t[left, :2] + (tau / dt)[:, None] * (t[left + 1, :2] - t[left, :2])      # (0.1 m steps: the chord is the path to 1e-4 m)
    z = np.linalg.norm(p["landmark_truth"][lm] - at, axis=1) + 0.5 * rng.standard_normal(M)
    bad = rng.permutation(M)[:13]
    if outliers:
        z[bad] += 5.0
    keep = np.ones(M, dtype=bool) if outliers else ~np.isin(np.arange(M), bad)
    p.update(range_left=left[keep], range_lm=lm[keep], range_z=z[keep], range_sigma=np.full(int(keep.sum()), 0.5),
             range_dt=np.full(int(keep.sum()), dt), range_tau=tau[keep])
    return p, bad


def test_huber_converges_and_moves_the_answer_towards_the_outlier_free_one():
    gp = gpu()
    p, bad = _plaza()
    clean, _ = _plaza(outliers=False)
    mk = lambda q: S.apply(q, gp.ChainSolver(O.POSE2, gp.CHART_FIRST_ORDER, 2))
    k = 1.345

    def robustify(s):
        s.set_meas_robust(0, np.full(M, gp.chain.ROBUST_HUBER, dtype=np.int32), np.full(M, k))
        s.compile()
        return s
    # every accepted Levenberg-Marquardt call lowers the robust cost
    it = robustify(mk(p))
    lam, accepted = 1e-5, 0
    for _ in range(12):
        rc, st, lam = it.iterate_lm(lam)
        assert rc == 0
        if st.accepted:
            accepted += 1
            assert st.error_after <= st.error_before, (st.error_before, st.error_after)
    assert accepted >= 3
    it.close()
    # optimize() under the ordinary stop rules (tolerances tight enough for the |delta| < 1e-6 statement below)
    sols = {}
    for name, q, rob in (("robust", p, True), ("plain", p, False), ("clean", clean, False)):
        s = mk(q)
        if rob:
            s = robustify(s)
        prm = s.default_params(use_lm=1, relative_error_tol=1e-13, absolute_error_tol=1e-13, max_iterations=200)
        rc, st = s.optimize(prm)
        assert rc == 0 and st.iterations < 200, (name, st.iterations)
        assert st.error_after <= st.error_before
        sols[name] = (s.get_states(), s.get_landmarks(), st.iterations, st.error_after)
        if rob:
            wts = s.meas_weights(0, M)
        s.close()
    # stationarity of sum rho: the reweighted plain handle at the final states has nothing left to do
    (xr, vr), lr = sols["robust"][0], sols["robust"][1]
    q = dict(p, pose=xr, vel=vr, landmarks=lr)
    h = mk(q)
    e, _ = h.linearize_meas(0, M)
    r = np.abs(e[:, 0]) / 0.5
    h.close()
    w, _ = np_loss("HUBER", k, r)
    assert np.abs(w - wts).max() <= 1e-13
    q["range_sigma"] = 0.5 / np.sqrt(w)
    h = mk(q)
    rc, st = h.iterate_gn()
    h.close()
    d_rob = np.linalg.norm(sols["robust"][0][0][:, :2] - sols["clean"][0][0][:, :2], axis=1).max()
    d_plain = np.linalg.norm(sols["plain"][0][0][:, :2] - sols["clean"][0][0][:, :2], axis=1).max()
    print("plaza: iterations %s, final step of the reweighted plain handle %.3e, max position distance to the outlier-free solution: robust %.4f m, plain %.4f m; "
          "weights of the 13 displaced ranges %s, smallest other weight %.3f" % ({n: v[2] for n, v in sols.items()}, st.delta_inf_norm, d_rob, d_plain,
                                                                                 np.round(np.sort(wts[bad]), 3), np.delete(wts, bad).min()))
    assert rc == 0 and st.delta_inf_norm < 1e-6, st.delta_inf_norm
    assert d_rob < d_plain, (d_rob, d_plain)


# ---------------------------------------------------------------- 5. forms and refusals
def test_robust_gps_takes_the_row_form_and_plain_gps_keeps_its_lines():
    gp = gpu()
    g, r, err, k = plain_side("interp-gps-pose3")
    plain = g.feed()
    rob = g.feed(loss=gp.chain.ROBUST_CAUCHY, k=k)
    assert plain.plan_info()["structured_gp"] == 2 and plain.plan_info()["fused"] == 1, plain.plan_info()
    assert rob.plan_info()["structured_gp"] == 1 and rob.plan_info()["fused"] == 1, rob.plan_info()
    for s in (plain, rob):
        s.launch_census()
        s.iterate_gn()
    cp, cr = plain.launch_census(), rob.launch_census()
    assert cp["gps_lines"] >= 1 and cp["lines"] == 1 and cp["sv"] == 4, cp
    assert cr["gps_lines"] == 0 and cr["lines"] == 0 and cr["meas_rec"] >= 1 and cr["sv"] == 3, cr
    plain.close()
    rob.close()


def test_refusals():
    gp = gpu()
    g, r, err, k = plain_side("interp-range-pose2")
    with pytest.raises(gp.GpslamHipError, match="robust.*fp32"):
        g.feed(loss=gp.chain.ROBUST_HUBER, k=k, precision=gp.FP32)
    with pytest.raises(gp.GpslamHipError, match="robust.*sharded"):
        g.feed(loss=gp.chain.ROBUST_HUBER, k=k, force_sharded=True)
    s = gp.ChainSolver(gp.ROT3_BIAS)
    with pytest.raises(gp.GpslamHipError, match="AHRS"):
        s.set_meas_robust(gp.chain.MEAS_AHRS, [gp.chain.ROBUST_HUBER], [1.0])
    s.close()
    s = g.feed()
    with pytest.raises(gp.GpslamHipError, match="positive and finite"):
        s.set_meas_robust(g.mk, [gp.chain.ROBUST_HUBER], [0.0])
    with pytest.raises(gp.GpslamHipError, match="unknown loss"):
        s.set_meas_robust(g.mk, [7], [1.0])
    with pytest.raises(gp.GpslamHipError, match="more losses than factors"):
        s.set_meas_robust(g.mk, np.ones(M + 1, dtype=np.int32), np.ones(M + 1))
    with pytest.raises(gp.GpslamHipError, match="more losses than factors"):
        s.set_between_pairs_robust([1], [1.0])
    # a setter call un-compiles the handle
    s.set_meas_robust(g.mk, [gp.chain.ROBUST_FAIR], [2.0])
    with pytest.raises(gp.GpslamHipError, match="compile"):
        s.error()
    s.compile()
    w = s.meas_weights(g.mk, M)
    assert np.all(w[:-1] == 1.0) and 0.0 < w[-1] < 1.0      # the most recently added factor carries the loss
    s.close()


# ---------------------------------------------------------------- 6. the segmented landmark path
@pytest.mark.parametrize("loss", ["HUBER"])
def test_segmented_landmark_path(loss):
    g, r, err, k = plain_side("interp-range-pose2")
    probe = g.feed(force_segmented=True, segment_length=35)
    assert probe.segment_plan()["active"] == 1
    probe.close()
    check_identity(g, r, err, k, loss, rows=False, force_segmented=True, segment_length=35)


# ---------------------------------------------------------------- 7. the folded retraction
def test_run_gn_equals_single_iterations_on_a_robust_graph():
    gp = gpu()
    g, r, err, k = plain_side("odometry2d-linear3")
    a = g.feed(loss=gp.chain.ROBUST_HUBER, k=k)
    b = g.feed(loss=gp.chain.ROBUST_HUBER, k=k)
    for _ in range(4):
        _, sa = a.iterate_gn()
    sb, _ = b.run_gn(4)
    (xa, va), (xb, vb) = a.get_states(), b.get_states()
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert (sa.error_before, sa.error_after, sa.delta_inf_norm) == (sb.error_before, sb.error_after, sb.delta_inf_norm)
    a.close()
    b.close()
