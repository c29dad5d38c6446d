"""Fixed-lag smoothing with landmarks on the device (gpslam_amd/csrc/fixedlag.hip: gpslam_hip_add_border_gaussians,
gpslam_hip_marginalize_head_onto_landmarks) against the oracle's arrays and the numpy model of tests/fixed_lag_border_model.py.

Graphs (fixed_lag_border_model.border_problem): tests/test_gpu_fixed_lag.problem(name, 12, k)'s chain plus two ranges per interval
(sigma 0.1) and landmark priors (sigma 0.5); one landmark seen only from the head, one only from the tail, one by the factor on
(k - 1, k).  SE(2) with an interpolated and a plain range and 3 landmarks; SE(2) with 13 landmarks (R = 27); SE(3) with interpolated
ranges to 9 landmarks (R = 28); the 2-D linear chain (block size 6) with its interpolated range.

Tolerance of Lambda / gamma (lam_tol, the rule of tests/test_gpu_fixed_lag.py): 100 x the largest distance, over the cases of
test_lambda_gamma, between the model run in float64 and in np.longdouble on the oracle's float64 normal equations, relative to
max |diag| of the head's share of [D_k^left ; H_LL^head] (gamma: max |g|, |g_L|); asserted to stay below 1e-10.  Blocks of the normal
equations are compared at 1e-11 of the largest entry of the reference array (D's entries reach 1e5 on these chains).  States and
landmarks after a step: 1e-9, the project's per-step bound.  Marginals: 1e-9 of sigma_i sigma_j, the bound of tests/test_gpu_marginals.py."""
import functools

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import synthetic as S
from oracle import oracle as O
from helpers import pose_close
import fixed_lag_border_model as FB

pytestmark = pytest.mark.gpu
E = O.CHART_EXPMAP
# name, landmarks, plain range factors beside the interpolated ones
GRAPHS = {"pose2": ("pose2", 3, True), "pose2_wide": ("pose2", 13, True), "pose3": ("pose3", 9, False), "linear3": ("linear3", 3, False)}


def graph(g, k, N=12, **kw):
    name, L, plain = GRAPHS[g]
    return FB.border_problem(name, N, k, L, plain=plain, **kw)


def solver(p, onto=True, **kw):
    dev = FB.apply(p, gp.ChainSolver(p["kind"], landmark_dim=FB.LD[p["kind"]], **kw))
    if onto:
        dev.marginalize_head_onto_landmarks()
    return dev


def check(kind, dev, rp, rv, rl, tol=1e-9):
    dp, dv = dev.get_states()
    assert np.abs(dv - rv).max() <= tol
    for a, b in zip(dp, rp):
        assert pose_close(kind, a, b, tol)
    assert np.abs(dev.get_landmarks() - rl).max() <= tol


def prior_of(dev):
    idx, pl, vl, ll, A, c = dev.get_border_gaussians()
    return [(int(idx[f]), pl[f], vl[f], ll[f].reshape(dev.L, dev.ld), A[f], c[f]) for f in range(len(idx))]


# ---------------------------------------------------------------- 1. the factor
@pytest.mark.parametrize("chart", [0, 1])
def test_border_gaussian_error_and_normal_equations(chart):
    p = graph("pose2", 2, N=4)
    kind, N, b = p["kind"], 4, 6
    rng = np.random.default_rng(12)
    orc = FB.apply(p, O.Chain(kind, chart=chart, landmark_dim=2))
    dev = FB.apply(p, gp.ChainSolver(kind, chart=chart, landmark_dim=2))
    nl = 6
    n = b + nl
    idx = np.array([0, N - 1], dtype=np.int32)
    lin_p = np.stack([O.retract(kind, p["pose"][i], 0.3 * rng.standard_normal(3), chart) for i in idx])
    lin_v = p["vel"][idx] + 0.3 * rng.standard_normal((2, 3))
    lin_l = p["landmarks"][None] + 0.3 * rng.standard_normal((2, 3, 2))
    A, c = rng.standard_normal((2, n, n)), rng.standard_normal((2, n))
    A[1, 3:7] = 0.0          # zero rows are the normal case
    dev.add_border_gaussians(idx, lin_p, lin_v, lin_l, A, c)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-4\)"):
        dev.error()
    dev.compile()
    for a, e in zip(dev.get_border_gaussians(), (idx, lin_p, lin_v, lin_l.reshape(2, nl), A, c)):
        assert np.array_equal(a, e)
    assert dev.get_rows()[0].shape[0] == orc_rows(p)      # no rows of its own
    gaussians = [(int(idx[f]), lin_p[f], lin_v[f], lin_l[f], A[f], c[f]) for f in range(2)]
    H, rhs, err = FB.system(orc, kind, chart, gaussians)
    assert abs(dev.error() - err) <= 1e-11 * err
    D, Om, g, B = dev.normal_equations()
    for i in (0, N - 1):
        s = slice(i * b, (i + 1) * b)
        for got, ref, scale in ((D[i], H[s, s], np.abs(H[:N * b, :N * b]).max()), (g[i], rhs[s], np.abs(rhs).max()),
                                (B[i], H[s, N * b:], np.abs(H[:N * b, N * b:]).max())):
            assert np.abs(got - ref).max() <= 1e-11 * scale
    # ... and the factor's own share, held to 1e-11 of ITS largest entry: the device's arrays with the factor minus the same handle's
    # without it (the factor is added to the assembled record, so the base is the same to the bit).  The sum itself is rounded once
    # at the size of the block's entries, which no implementation avoids: that rounding, eps of the block's largest entry, is added.
    base = FB.apply(p, gp.ChainSolver(kind, chart=chart, landmark_dim=2))
    D0, _, g0, B0 = base.normal_equations()
    H0, rhs0, _ = FB.system(orc, kind, chart, [])
    eps = np.finfo(float).eps
    for i in (0, N - 1):
        s = slice(i * b, (i + 1) * b)
        for got, had, ref in ((D[i], D0[i], H[s, s] - H0[s, s]), (g[i], g0[i], rhs[s] - rhs0[s]), (B[i], B0[i], H[s, N * b:] - H0[s, N * b:])):
            assert np.abs(ref).max() > 0.1
            assert np.abs((got - had) - ref).max() <= 1e-11 * np.abs(ref).max() + 4 * eps * np.abs(got).max()
    dev.clear_factors()
    assert dev.get_border_gaussians()[0].size == 0


def orc_rows(p):
    d = O.TANGENT_DIM[p["kind"]]
    return (2 * d * len(p["gp_left"]) + d * (len(p["prior_idx"]) + len(p["vprior_idx"]) + len(p["between_left"])) + len(p["range_left"])
            + len(p.get("prange_idx", ())))


def test_block_diagonal_border_gaussian_is_state_gaussian_plus_landmark_priors():
    p = graph("pose2", 5, lpriors=False)
    rng = np.random.default_rng(4)
    L, b = 3, 6
    Ax, cx = rng.standard_normal((b, b)), rng.standard_normal(b)
    sig = 0.3 + rng.random((L, 2))
    at = p["landmarks"] + 0.2
    a, bdev = solver(p, onto=False), solver(p, onto=False)
    a.add_state_gaussians([3], p["pose"][3:4], p["vel"][3:4], Ax[None], cx[None])
    a.add_landmark_priors(np.arange(L), at, sig)
    A = np.zeros((b + 2 * L, b + 2 * L))
    A[:b, :b] = Ax
    A[b:, b:] = np.diag(1.0 / sig.reshape(-1))
    bdev.add_border_gaussians([3], p["pose"][3:4], p["vel"][3:4], at[None], A[None], np.concatenate([cx, np.zeros(2 * L)])[None])
    for s in (a, bdev):
        s.compile()
    assert abs(a.error() - bdev.error()) <= 1e-11 * a.error()
    for s in (a, bdev):
        s.iterate_gn()
    pa, va = a.get_states()
    check(p["kind"], bdev, pa, va, a.get_landmarks(), 1e-11)


# ---------------------------------------------------------------- 2. Lambda, gamma
LG_CASES = [(g, k) for g in GRAPHS for k in (1, 2, 5, 11)]


def head_reference(p, k, dtype=np.float64):
    return FB.schur_border(*FB.head_arrays(p, k), k, dtype)


@functools.lru_cache(maxsize=None)
def lam_tol():
    worst = 0.0
    for g, k in LG_CASES:
        p = graph(g, k)
        L0, g0, sD, sg = head_reference(p, k)
        L1, g1, _, _ = head_reference(p, k, np.longdouble)
        worst = max(worst, float(np.abs(L0 - L1).max()) / sD, float(np.abs(g0 - g1).max()) / sg)
    tol = 100.0 * worst
    print("model float64 against longdouble: %.3g relative; tolerance %.3g" % (worst, tol))
    assert 0.0 < tol < 1e-10
    return tol


@pytest.mark.parametrize("g,k", LG_CASES)
def test_lambda_gamma(g, k):
    tol = lam_tol()
    p = graph(g, k)
    dev = solver(p)
    b = dev.b
    dev.marginalize_head(k)
    assert dev.N == 12 - k
    ll, Lam, gam = dev.get_head_prior_border()
    pl, vl, Lxx, gx = dev.get_head_prior()
    assert np.array_equal(pl, p["pose"][k]) and np.array_equal(vl, p["vel"][k]) and np.array_equal(ll, p["landmarks"])
    assert np.array_equal(Lxx, Lam[:b, :b]) and np.array_equal(gx, gam[:b])
    L0, g0, sD, sg = head_reference(p, k)
    eL, eg = float(np.abs(Lam - L0).max()) / sD, float(np.abs(gam - g0).max()) / sg
    print("%s k = %d: device against model %.3g (Lambda), %.3g (gamma) relative; tolerance %.3g" % (g, k, eL, eg, tol))
    assert eL <= tol and eg <= tol
    (idx, pl2, vl2, ll2, A, c), = [dev.get_border_gaussians()]
    assert list(idx) == [0] and dev.get_state_gaussians()[0].size == 0
    assert np.array_equal(pl2[0], pl) and np.array_equal(vl2[0], vl) and np.array_equal(ll2[0], ll.reshape(-1))
    assert np.abs(A[0].T @ A[0] - 0.5 * (Lam + Lam.T)).max() <= 1e-11 * sD
    assert np.abs(A[0].T @ c[0] + gam).max() <= 1e-11 * sg
    assert (np.abs(A[0]).max(axis=1) == 0.0).any()         # Lambda is rank-deficient: landmark 1 is not seen from the head


# ---------------------------------------------------------------- 3. one step equals batch, more steps and LM track the model
@pytest.mark.parametrize("g,k", [("pose2", 1), ("pose2", 5), ("pose2_wide", 5), ("pose3", 2), ("pose3", 11), ("linear3", 5)])
def test_one_step_equals_batch_then_tracks_the_model(g, k):
    p = graph(g, k)
    kind = p["kind"]
    orc = FB.apply(p, FB.chain(p))
    dev = solver(p)
    dev.marginalize_head(k)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-4\)"):
        dev.iterate_gn()
    dev.compile()
    orc.iterate_gn()
    dev.iterate_gn()
    bp, bv = orc.get_states()
    check(kind, dev, bp[k:], bv[k:], orc.get_landmarks())
    # more steps: the model's dense iteration on the tail-only oracle chain with the device's prior
    _, tail = FB.head_tail(p, k)
    tail["pose"], tail["vel"] = dev.get_states()
    tail["landmarks"] = dev.get_landmarks()
    ref = FB.apply(tail, FB.chain(tail))
    prior = prior_of(dev)
    for _ in range(3):
        rp, rv, rl, _ = FB.step(ref, kind, E, prior)
        dev.iterate_gn()
        check(kind, dev, rp, rv, rl)


@pytest.mark.parametrize("g,k", [("pose2", 1), ("pose2_wide", 5), ("pose3", 2), ("linear3", 5)])
def test_one_lm_iteration_is_the_models_damped_step(g, k):
    """iterate_lm at a fixed lambda, from the states the head was marginalised at (the step is of the size of the initial error, so
    the trial is accepted on its merits): the model's damped step (H + lambda I) and the error behind it"""
    p = graph(g, k)
    kind = p["kind"]
    dev = solver(p)
    dev.marginalize_head(k)
    dev.compile()
    _, tail = FB.head_tail(p, k)
    ref = FB.apply(tail, FB.chain(tail))
    prior = prior_of(dev)
    lam = 0.5
    err0 = FB.system(ref, kind, E, prior)[2]
    assert abs(dev.error() - err0) <= 1e-11 * err0
    rp, rv, rl, err = FB.step(ref, kind, E, prior, lam)
    _, st, _ = dev.iterate_lm(lam)
    assert st.accepted == 1 and st.trials == 1
    check(kind, dev, rp, rv, rl)
    assert abs(st.error_after - err) <= 1e-9 * max(1.0, err) and abs(dev.error() - err) <= 1e-9 * max(1.0, err)


@pytest.mark.parametrize("g,k", [("pose2", 5), ("pose3", 2)])
def test_lm_model_fidelity_sees_the_factors_gradient(g, k):
    """Levenberg-Marquardt's model decrease is delta . g / 2 + lambda |delta|^2 / 2 with g from the gradient copy and g_L: both must
    carry the border Gaussian's share.  The model computes the fidelity rho of the first trial with the whole gradient and with
    the factor's share left out; with min_model_fidelity between the two, the first trial is accepted exactly when the true rho is
    the larger one."""
    p = graph(g, k)
    kind = p["kind"]
    dev = solver(p)
    dev.marginalize_head(k)
    dev.compile()
    _, tail = FB.head_tail(p, k)
    ref = FB.apply(tail, FB.chain(tail))
    prior = prior_of(dev)
    lam = 0.5
    H, rhs, err0 = FB.system(ref, kind, E, prior)
    rhs_without = FB.system(ref, kind, E, [])[1]
    delta = np.linalg.solve(H + lam * np.eye(H.shape[0]), rhs)
    err1 = FB.step(ref, kind, E, prior, lam)[3]
    rho = (err0 - err1) / (0.5 * delta @ rhs + 0.5 * lam * delta @ delta)
    rho_without = (err0 - err1) / (0.5 * delta @ rhs_without + 0.5 * lam * delta @ delta)
    print("%s k = %d: rho %.4f, without the factor's gradient %.4f" % (g, k, rho, rho_without))
    # the probe needs the two apart by far more than rho is uncertain: errors agree with the model at 1e-9 relative, and the error
    # decrease is of the error's own size here, so the device's rho is the model's to about 1e-8
    assert abs(rho - rho_without) > 1e-4
    thr = 0.5 * (rho + rho_without)
    _, st, _ = dev.iterate_lm(lam, dev.default_params(use_lm=1, min_model_fidelity=thr))
    assert (st.trials == 1 and st.accepted == 1) == (rho > thr)


@pytest.mark.parametrize("g,k,lam", [("pose2", 5, 50.0), ("pose3", 2, 0.5)])
def test_lm_second_trial_after_a_rejected_first(g, k, lam):
    """A rejected trial must leave the factor's linearisation residual alone: the second trial re-assembles from it.  The model
    computes the fidelity rho of the trials at lam and at 10 lam (the second is the larger on these graphs); with min_model_fidelity
    between the two the first trial is rejected and the second accepted, and the states, landmarks and error are the model's damped
    step at 10 lam from the linearisation point."""
    p = graph(g, k)
    kind = p["kind"]
    dev = solver(p)
    dev.marginalize_head(k)
    dev.compile()
    _, tail = FB.head_tail(p, k)
    prior = prior_of(dev)
    rho, out = [], None
    for l in (lam, 10.0 * lam):
        ref = FB.apply(tail, FB.chain(tail))
        H, rhs, err0 = FB.system(ref, kind, E, prior)
        delta = np.linalg.solve(H + l * np.eye(H.shape[0]), rhs)
        out = FB.step(ref, kind, E, prior, l)
        rho.append((err0 - out[3]) / (0.5 * delta @ rhs + 0.5 * l * delta @ delta))
    print("%s k = %d: rho %.6f at lambda %g, %.6f at %g" % (g, k, rho[0], lam, rho[1], 10.0 * lam))
    assert rho[1] - rho[0] > 1e-5          # (far above what rho is uncertain by: about 1e-8, see the probe above)
    _, st, _ = dev.iterate_lm(lam, dev.default_params(use_lm=1, min_model_fidelity=0.5 * (rho[0] + rho[1]), lambda_factor=10.0))
    assert st.trials == 2 and st.accepted == 1
    rp, rv, rl, err = out
    check(kind, dev, rp, rv, rl)
    assert abs(st.error_after - err) <= 1e-9 * max(1.0, err) and abs(dev.error() - err) <= 1e-9 * max(1.0, err)


# ---------------------------------------------------------------- 4. with a loop closure in the tail
def test_one_step_with_a_loop_closure_in_the_tail():
    k = 3
    p = S.add_loop_closures(graph("pose2", k), [(k + 1, 10)])
    orc = FB.apply(p, FB.chain(p))
    dev = solver(p)
    dev.marginalize_head(k)
    dev.compile()
    orc.iterate_gn()
    dev.iterate_gn()
    bp, bv = orc.get_states()
    check(p["kind"], dev, bp[k:], bv[k:], orc.get_landmarks())


# ---------------------------------------------------------------- 5. twice equals once
@pytest.mark.parametrize("g", ["pose2", "pose3"])
def test_marginalising_twice_equals_once(g):
    p = graph(g, 5)
    a, b = solver(p), solver(p)
    a.marginalize_head(2)
    a.compile()
    a.marginalize_head(3)
    b.marginalize_head(5)
    for s in (a, b):
        s.compile()
        s.iterate_gn()
    assert [int(i) for i in a.get_border_gaussians()[0]] == [0]
    pb, vb = b.get_states()
    check(p["kind"], a, pb, vb, b.get_landmarks())


# ---------------------------------------------------------------- 6. a head without absolute information
def test_gauge_free_head():
    k = 4
    p = graph("pose2", k, priors=False)
    at = np.array([k + 2, 10], dtype=np.int32)
    p.update(prior_idx=at, prior_pose=p["pose"][at] + 0.05, prior_sig=np.full((2, 3), 0.05))
    orc = FB.apply(p, FB.chain(p))
    dev = solver(p)
    dev.marginalize_head(k)          # no GPSLAM_E_NOT_SPD
    dev.compile()
    orc.iterate_gn()
    dev.iterate_gn()
    bp, bv = orc.get_states()
    check(p["kind"], dev, bp[k:], bv[k:], orc.get_landmarks())


# ---------------------------------------------------------------- 7. marginals
@pytest.mark.parametrize("g", ["pose2", "pose3"])
def test_marginals_with_a_border_gaussian(g):
    k = 5
    p = graph(g, k)
    kind = p["kind"]
    dev = solver(p)
    dev.marginalize_head(k)
    dev.compile()
    dev.marginals()
    Sd, Sn, Slm, Sxl = dev.get_marginals(cross=True)
    _, tail = FB.head_tail(p, k)
    ref = FB.apply(tail, FB.chain(tail))
    C = FB.dense_marginals(ref, kind, E, prior_of(dev))
    N, b = dev.N, dev.b
    sd = np.sqrt(np.diag(C))
    worst = 0.0
    for i in range(N):
        s, s1 = slice(i * b, (i + 1) * b), slice((i + 1) * b, (i + 2) * b)
        worst = max(worst, (np.abs(Sd[i] - C[s, s]) / np.outer(sd[s], sd[s])).max())
        if i + 1 < N:
            worst = max(worst, (np.abs(Sn[i] - C[s, s1]) / np.outer(sd[s], sd[s1])).max())
        worst = max(worst, (np.abs(Sxl[i] - C[s, N * b:]) / np.outer(sd[s], sd[N * b:])).max())
    worst = max(worst, (np.abs(Slm - C[N * b:, N * b:]) / np.outer(sd[N * b:], sd[N * b:])).max())
    print("%s: marginals against the dense inverse %.3g of sigma_i sigma_j" % (g, worst))
    assert worst <= 1e-9


# ---------------------------------------------------------------- 8. a sliding window
def test_sliding_window_tracks_the_model():
    """16 states, a window of 8 slid by 2 four times; after each slide (marginalise, append, the new factors, one Gauss-Newton step)
    the device against the model's step on the window's tail factors plus the device's prior."""
    N, W, step = 16, 8, 2
    p = FB.border_problem("pose2", N, 7, 3)
    kind = p["kind"]
    keys = FB.FACTOR_KEYS

    def window(lo, hi, new_from=None):
        out = dict(kind=kind, qc=p["qc"], N=hi - lo, pose=p["pose"][lo:hi].copy(), vel=p["vel"][lo:hi].copy())
        for key in ("landmarks", "lprior_idx", "lprior", "lprior_sig"):
            out[key] = p[key]
        for key, (others, two) in keys.items():
            if key not in p:
                continue
            idx = np.asarray(p[key])
            last = idx + (1 if two else 0)
            m = (idx >= lo) & (last < hi)
            if new_from is not None:
                m &= last >= new_from
            out[key] = (idx[m] - lo).astype(np.int32)
            for o in others:
                out[o] = np.asarray(p[o])[m]
        return out

    dev = solver(window(0, W))
    dev.iterate_gn()
    lo, hi = 0, W
    for _ in range(4):
        dev.marginalize_head(step)
        dev.append_states(p["pose"][hi:hi + step], p["vel"][hi:hi + step])
        new = window(lo + step, hi + step, new_from=hi)
        dev.add_gp_priors(new["gp_left"], new["gp_dt"])
        dev.add_pose_priors(new["prior_idx"], new["prior_pose"], new["prior_sig"])
        dev.add_between(new["between_left"], new["between_meas"], new["between_sig"])
        dev.add_interp_range(new["range_left"], new["range_lm"], new["range_z"], new["range_sigma"], new["range_dt"], new["range_tau"])
        dev.add_range(new["prange_idx"], new["prange_lm"], new["prange_z"], new["prange_sigma"])
        lo, hi = lo + step, hi + step
        dev.compile()
        # the model: every factor inside the window that is not in the marginalised head, plus the device's prior
        tail = window(lo, hi)
        tail["pose"], tail["vel"] = dev.get_states()
        tail["landmarks"] = dev.get_landmarks()
        ref = FB.apply(tail, FB.chain(tail))
        prior = prior_of(dev)
        assert len(prior) == 1 and prior[0][0] == 0
        rp, rv, rl, _ = FB.step(ref, kind, E, prior)
        dev.iterate_gn()
        check(kind, dev, rp, rv, rl)
    assert hi == N and dev.N == W


# ---------------------------------------------------------------- 9. / 10. the contract
def run3(dev):
    for _ in range(3):
        dev.iterate_gn()
    return dev.get_states() + (dev.get_landmarks(),)


def same(a, b):
    for x, y in zip(run3(a), run3(b)):
        assert np.array_equal(x, y)


def test_option_off_refuses_as_before():
    p = graph("pose2", 5)
    twin, dev = solver(p, onto=False), solver(p, onto=False)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*is in the head and names landmark \d+: the prior would span the state and that landmark"):
        dev.marginalize_head(5)
    dev.marginalize_head_onto_landmarks(True)
    dev.marginalize_head_onto_landmarks(False)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*the prior would span the state and that landmark"):
        dev.marginalize_head(5)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\)"):
        dev.get_head_prior_border()
    assert dev.N == 12
    same(twin, dev)


def test_refusals_leave_the_handle_as_it_was():
    p = graph("pose2", 5)
    twin, dev = solver(p), solver(p)
    for k in (0, 12, -3):
        with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\)"):
            dev.marginalize_head(k)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\)"):
        dev.get_head_prior_border()
    n = dev.b + 6
    bad = np.eye(n)[None].copy()
    bad[0, 2, 3] = np.nan
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\)"):
        dev.add_border_gaussians([0], p["pose"][:1], p["vel"][:1], p["landmarks"][None], bad, np.zeros((1, n)))
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\)"):
        dev.add_border_gaussians([0], p["pose"][:1], p["vel"][:1], p["landmarks"][None] * np.inf, np.eye(n)[None], np.zeros((1, n)))
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\)"):
        dev.add_border_gaussians([12], p["pose"][:1], p["vel"][:1], p["landmarks"][None], np.eye(n)[None], np.zeros((1, n)))
    assert dev.N == 12 and dev.get_border_gaussians()[0].size == 0
    same(twin, dev)
    # a loop closure that reaches into the head
    pc = S.add_loop_closures(p, [(1, 9)])
    twin, dev = solver(pc), solver(pc)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*reaches into the head"):
        dev.marginalize_head(3)
    assert dev.N == 12
    same(twin, dev)
    # a border Gaussian in the head with the option off (on a graph whose first states see no landmark)
    q = dict(p)
    for key in ("range_left", "prange_idx"):
        m = np.asarray(p[key]) >= 3
        q[key] = np.asarray(p[key])[m]
        for o in FB.FACTOR_KEYS[key][0]:
            q[o] = np.asarray(p[o])[m]
    twin, dev = solver(q, onto=False), solver(q, onto=False)
    for s in (twin, dev):
        s.add_border_gaussians([1], q["pose"][1:2], q["vel"][1:2], q["landmarks"][None], np.eye(n)[None], np.zeros((1, n)))
        s.compile()
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*border Gaussian 0"):
        dev.marginalize_head(2)
    assert dev.N == 12
    same(twin, dev)
    # no landmarks on the handle; a stored factor whose landmark count no longer matches
    q = {key: v for key, v in p.items() if not key.startswith(("landmarks", "lprior", "range_", "prange_"))}
    plain = S.apply(q, gp.ChainSolver(q["kind"]))
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\)"):
        plain.add_border_gaussians([0], q["pose"][:1], q["vel"][:1], np.zeros((1, 0)), np.eye(6)[None], np.zeros((1, 6)))
    same(S.apply(q, gp.ChainSolver(q["kind"])), plain)
    dev = solver(p)
    dev.add_border_gaussians([0], p["pose"][:1], p["vel"][:1], p["landmarks"][None], np.eye(n)[None], np.zeros((1, n)))
    dev.set_landmarks(p["landmarks"][:2])
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\)"):
        dev.compile()


@pytest.mark.parametrize("what", ["fp32", "sharded", "segmented"])
def test_unsupported_handles_refuse(what):
    if what == "segmented":
        p = dict(S.pose2_range_chain(60, L=8, seed=1))
        p["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
        kw = dict(force_segmented=True)
    else:
        p = graph("pose2", 5)
        kw = dict(precision=gp.chain.FP32) if what == "fp32" else dict(force_sharded=True)
    twin, dev = solver(p, **kw), solver(p, **kw)
    n = dev.b + 2 * dev.L
    N = dev.N
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*" + what):
        dev.marginalize_head(3)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*" + what):
        dev.add_border_gaussians([0], p["pose"][:1], p["vel"][:1], p["landmarks"][None], np.eye(n)[None], np.zeros((1, n)))
    assert dev.N == N
    same(twin, dev)


def test_a_piece_of_a_split_chain_is_refused():
    """A piece iterates only through its driver's phases with the other pieces, so there is no twin to iterate against (as in
    tests/test_gpu_fixed_lag.py): the answers, and the states and factors as they were."""
    p = graph("pose2", 5)
    h = gp.ChainSolver(O.POSE2, landmark_dim=2)
    h.set_states(p["pose"], p["vel"])
    h.set_landmarks(p["landmarks"])
    h.fs_set_split(0, 2)
    h.marginalize_head_onto_landmarks()
    n = h.b + 6
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*split"):
        h.marginalize_head(3)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*split"):
        h.add_border_gaussians([0], p["pose"][:1], p["vel"][:1], p["landmarks"][None], np.eye(n)[None], np.zeros((1, n)))
    pose, vel = h.get_states()
    assert np.array_equal(pose, p["pose"]) and np.array_equal(vel, p["vel"]) and h.get_border_gaussians()[0].size == 0


def test_rot3_bias_is_refused():
    pb = S.rot3_bias_ahrs_chain(12)
    lm = np.array([[1.0, 2.0], [3.0, -1.0]])

    def make():
        h = gp.ChainSolver(pb["kind"], landmark_dim=2)
        h.set_landmarks(lm)
        S.apply(pb, h)
        h.add_landmark_priors([0, 1], lm + 0.1, np.full((2, 2), 0.5))
        h.compile()
        h.marginalize_head_onto_landmarks()
        return h
    twin, hb = make(), make()
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*ROT3_BIAS"):
        hb.marginalize_head(3)
    assert hb.N == 12
    same(twin, hb)
    n = hb.b + 4
    hb.add_border_gaussians([0], pb["pose"][:1], pb["vel"][:1], lm[None], np.eye(n)[None], np.zeros((1, n)))
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*border Gaussians.*ROT3_BIAS"):
        hb.compile()


def test_compile_refuses_border_gaussians_beyond_the_dense_border():
    """20 planar landmarks (nl = 40) take the segmented landmark path at compile(): the factor is stored, compile() says no"""
    p = dict(S.pose2_range_chain(60, L=20, seed=1))
    p["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
    twin, dev = solver(p), solver(p)
    assert dev.segment_plan()["active"] == 1
    n = dev.b + 40
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*segmented"):
        dev.add_border_gaussians([0], p["pose"][:1], p["vel"][:1], p["landmarks"][None], np.eye(n)[None], np.zeros((1, n)))
    same(twin, dev)
    raw = gp.ChainSolver(O.POSE2, landmark_dim=2)          # before the first compile() nothing says "segmented" yet
    raw.set_landmarks(p["landmarks"])
    raw.set_qc(p["qc"]); raw.set_states(p["pose"], p["vel"]); raw.add_gp_priors(p["gp_left"], p["gp_dt"])
    raw.add_pose_priors(p["prior_idx"], p["prior_pose"], p["prior_sig"])
    raw.add_border_gaussians([0], p["pose"][:1], p["vel"][:1], p["landmarks"][None], np.eye(n)[None], np.zeros((1, n)))
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*border Gaussians.*segmented"):
        raw.compile()


def test_closures_in_column_passes_are_refused():
    """border Gaussians do not ride through the column passes of the closures: compile() and marginalize_head say so, and the
    handle iterates as its twin"""
    k = 3
    p = S.add_loop_closures(graph("pose2", k), [(k + 1, 10), (k + 2, 9), (k + 1, 8), (k + 3, 11)])

    def make():
        h = gp.ChainSolver(p["kind"], landmark_dim=2)
        h.set_closure_passes(8, 2)
        h.marginalize_head_onto_landmarks()
        return FB.apply(p, h)
    twin, dev = make(), make()
    assert dev.closure_info()["passes"] > 1
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*column passes"):
        dev.marginalize_head(k)
    assert dev.N == 12
    same(twin, dev)
    n = dev.b + 6
    dev.add_border_gaussians([0], p["pose"][:1], p["vel"][:1], p["landmarks"][None], np.eye(n)[None], np.zeros((1, n)))
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*border Gaussians.*column passes"):
        dev.compile()


def test_getters_refuse_when_the_landmark_count_changed():
    """the getters copy n = b + nl of the stored factors; a caller sizes its arrays from the handle's landmarks"""
    p = graph("pose2", 5)
    dev = solver(p)
    dev.marginalize_head(5)
    dev.set_landmarks(p["landmarks"][:2])
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\).*another number of landmarks"):
        dev.get_border_gaussians()
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\).*another number of landmarks"):
        dev.get_head_prior_border()
    dev.set_landmarks(p["landmarks"])
    assert dev.get_border_gaussians()[4].shape == (1, 12, 12) and dev.get_head_prior_border()[1].shape == (12, 12)


def test_block_size_4_keeps_the_state_prior():
    """The 2-D linear chain (block size 4) has no factor that names a landmark: with the option on, the head still leaves a state
    Gaussian, and one step equals the batch step"""
    k, N = 3, 9
    from test_gpu_fixed_lag import problem
    p = dict(problem("linear2", N, k))
    lm = np.array([[1.0, 2.0], [3.0, -1.0]])
    orc, dev = O.Chain(O.LINEAR2, landmark_dim=2), gp.ChainSolver(O.LINEAR2, landmark_dim=2)
    for s_ in (orc, dev):
        s_.set_landmarks(lm)
        S.apply(p, s_)
        s_.add_landmark_priors([0, 1], lm + 0.1, np.full((2, 2), 0.5))
        s_.compile()
    dev.marginalize_head_onto_landmarks()
    dev.marginalize_head(k)
    assert dev.get_state_gaussians()[0].size == 1 and dev.get_border_gaussians()[0].size == 0
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\)"):
        dev.get_head_prior_border()
    dev.compile()
    orc.iterate_gn()
    dev.iterate_gn()
    bp, bv = orc.get_states()
    check(O.LINEAR2, dev, bp[k:], bv[k:], orc.get_landmarks())


# ---------------------------------------------------------------- 11. reruns
def test_reruns_are_bit_identical():
    p = graph("pose3", 5)
    out = []
    for _ in range(2):
        dev = solver(p)
        dev.marginalize_head(5)
        dev.compile()
        dev.iterate_gn()
        dev.iterate_lm(0.1)
        out.append(dev.get_head_prior_border() + dev.get_states() + (dev.get_landmarks(),))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
