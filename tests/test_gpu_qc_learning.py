"""The Qc statistic on the device (gpslam_hip_qc_statistic, gpslam_amd/csrc/qc_learn.hip) against the numpy model, and
evidence.learn_qc on the linear problem of the evidence tests.

Reference: A_ref from np.linalg.inv of the oracle's dense H at the device's states and the oracle's linearize_gp() there
(qc_learning_model.statistic).  Bound, entrywise, from the tolerances the project already holds: check_blocks holds S / S_next to
tol_of(H) relative to dg dg^T (dg = sqrt(diag Sigma)), the host and factor arithmetic to 1e-11, so
    |A - A_ref| <= tol_of(H) sum_i sum_k |J~_k| (dg_J dg_J^T) |J~_k|^T + 1e-11 (sum_i sum_k |e~_k| |e~_k|^T + |A_ref|).
The reference is computed a second way, Sigma from a Cholesky factor of H instead of inv, and must itself sit inside the bound."""
import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import evidence as EV
from gpslam_amd import synthetic as S
from oracle import oracle as O
import evidence_model as EM
import qc_learning_model as QM
from test_gpu_marginals import CHAINS, oracle_H, solver, gn, tol_of
from test_gpu_vw import build_vw_pair
from test_gpu_closure_passes import _device, _info, _pairs
from test_gpu_closure import _anchored, _strip_landmarks
from test_gpu_evidence import _census_counts, _linear_solver, _evidence_tol, linear_problem  # noqa: F401 (linear_problem: a fixture)
from test_gpu_marginals_segmented import _range60_pair
from test_qc_learning_model import H_STEP, directions, fd_pair, evidence_noise

pytestmark = pytest.mark.gpu
REL = 1e-11
NPW2 = 64       # priors per stage of k_qc_stat, the unit a workgroup takes (kQcStage); they reach the LDS in rounds of 16 (kQcRound)


def reference(orc, dev, left, dts, p=None, use=None, H=None):
    """(A_ref, n_f, bound) at the device's states"""
    if H is None:
        H = oracle_H(orc, dev, p)
    else:
        orc.set_states(*dev.get_states())
    e, Hq = orc.linearize_gp()
    tol = tol_of(H)
    A, n_f, cov_scale, err_scale = QM.statistic(np.linalg.inv(H), e, Hq, left, dts, dev.b, use)
    bound = tol * cov_scale + REL * (err_scale + np.abs(A))
    Linv = np.linalg.inv(np.linalg.cholesky(H))
    A2 = QM.statistic(Linv.T @ Linv, e, Hq, left, dts, dev.b, use)[0]
    assert np.all(np.abs(A2 - A) <= bound), (np.abs(A2 - A) / bound).max()
    return A, n_f, bound


def check(what, dev, ref):
    A_ref, n_ref, bound = ref
    A, n_f = dev.qc_statistic()
    print("%s: n_f %d, |A| %.3g, worst |A - A_ref| / bound %.3g (largest bound %.3g)" % (what, n_f, np.abs(A).max(), (np.abs(A - A_ref) / bound).max(), bound.max()))
    assert n_f == n_ref
    assert np.array_equal(A, A.T)
    assert np.all(np.abs(A - A_ref) <= bound), (A, A_ref, bound)
    return A, n_f


# ---------------------------------------------------------------- 1. chains
@pytest.mark.parametrize("name", sorted(k for k in CHAINS if k != "rot3_bias") + ["pose3_vw"])
def test_chain_statistic_every_manifold(name):
    if name == "pose3_vw":
        orc, dev, c, _ = build_vw_pair(130, 3)
        left, dts = np.arange(129), c["dt"]
    else:
        p = CHAINS[name]()
        dev = solver(p)
        orc = S.apply(p, O.Chain(p["kind"]))
        left, dts = p["gp_left"], p["gp_dt"]
    gn(dev, 3)
    dev.marginals()
    check(name, dev, reference(orc, dev, left, dts))


@pytest.mark.parametrize("N", [2, 3, 16, 17, 18, 257, NPW2, NPW2 + 1, NPW2 + 2])
def test_linear2_lengths(N):
    """one prior; chunk ends of the marginals and N - 1 = a round of 16 priors - 1, + 0, + 1; N - 1 = one stage's priors - 1, + 0, + 1"""
    p = S.linear_chain(N, D=2, every=3)
    dev = solver(p)
    orc = S.apply(p, O.Chain(O.LINEAR2))
    gn(dev, 1)
    dev.marginals()
    check("linear2 N = %d" % N, dev, reference(orc, dev, p["gp_left"], p["gp_dt"]))


def test_linear2_chain_of_257_workgroups():
    """257 * 64 priors: k_qc_reduce adds 257 partials.  No dense inverse of 65796 x 65796: the reference takes Sigma_J from the
    device's own S / S_next (pinned to the model by tests/test_gpu_marginals.py), so the bound keeps its 1e-11 terms only, with
    sum |J~| |Sigma_J| |J~|^T in the place of the covariance scale"""
    N = 257 * NPW2 + 1
    p = S.linear_chain(N, D=2, every=3)
    dev = solver(p)
    orc = S.apply(p, O.Chain(O.LINEAR2))
    gn(dev, 1)
    dev.marginals()
    Sd, Sn = dev.get_marginals()
    orc.set_states(*dev.get_states())
    e, Hq = orc.linearize_gp()
    A_ref, n_f, cov_scale, err_scale = QM.statistic((Sd, Sn), e, Hq, p["gp_left"], p["gp_dt"], dev.b)
    assert n_f == 257 * NPW2
    check("linear2, 257 workgroups", dev, (A_ref, n_f, REL * (cov_scale + err_scale + np.abs(A_ref))))


def test_non_uniform_dt():
    p = dict(S.linear_chain(150, D=3))
    p["gp_dt"] = 0.05 + 0.15 * np.random.default_rng(7).random(149)
    dev = solver(p)
    orc = S.apply(p, O.Chain(O.LINEAR3))
    gn(dev, 2)
    dev.marginals()
    check("non-uniform dt", dev, reference(orc, dev, p["gp_left"], p["gp_dt"]))


# ---------------------------------------------------------------- 2. landmarks, closures, segments, mixed Qc
def test_plaza_like_pose2_first_order_chart_with_landmarks():
    """60 states: kappa of the Jacobi-scaled H is 1.2e6 (100 states: 9e6, beyond tol_of's cap of 4.5e6)"""
    p = _anchored(S.pose2_range_chain(60, L=4, seed=3))
    dev = solver(p, landmark_dim=2, chart=gp.CHART_FIRST_ORDER)
    orc = S.apply(p, O.Chain(O.POSE2, chart=O.CHART_FIRST_ORDER, landmark_dim=2))
    gn(dev, 2)
    dev.marginals()
    check("pose2, first-order chart, 4 landmarks", dev, reference(orc, dev, p["gp_left"], p["gp_dt"]))


@pytest.mark.parametrize("name", ["pose2_9", "pose2_12"])
def test_loop_closures_in_one_pass_and_in_column_passes(name):
    """the closure sets of test_gpu_evidence's cases of these names on the 60-state SE(2) base of test_gpu_marginals_passes (kappa
    5.6e5; the 150 states of the evidence cases: 5e7, beyond tol_of's cap): 9 closures in one pass, both chain ends among them, and
    12 in two column passes with the kept Z"""
    base = _anchored(_strip_landmarks(S.pose2_range_chain(60, seed=9)))
    if name == "pose2_9":
        p, kind, max_passes, info = S.add_loop_closures(base, [[0, 59], [59, 3], [1, 30]] + _pairs(60, 6, 21), seed=5), O.POSE2, None, (9, 9, 1)
    else:
        p, kind, max_passes, info = S.add_loop_closures(base, _pairs(60, 12, 21), seed=5), O.POSE2, 32, (12, 9, 2)
    dev = _device(p, max_passes)
    _info(dev, *info)
    if info[2] > 1:
        dev.marginals_keep_closure_columns()
    orc = S.apply(p, O.Chain(kind))
    gn(dev, 2)
    dev.marginals()
    check(name, dev, reference(orc, dev, p["gp_left"], p["gp_dt"], p=p))


def test_segmented_handle_with_marginals_on_segments():
    p, dense, seg, orc = _range60_pair()
    H = oracle_H(orc, dense)
    seg.marginals_on_segments()
    seg.marginals()
    print("plan %s" % seg.segment_plan())
    ref = reference(orc, seg, p["gp_left"], p["gp_dt"], H=H)
    A, _ = check("segmented, 60 states, 8 landmarks", seg, ref)
    dense.marginals()
    assert np.all(np.abs(dense.qc_statistic()[0] - A) <= 2 * ref[2])


def test_half_the_priors_keep_their_own_qc():
    """added as shared, own, shared: compile() reorders the device-side arrays by Qc, and the own-Qc priors are neither summed nor
    counted"""
    p = dict(S.linear_chain(120, D=3))
    left, dt = p["gp_left"], p["gp_dt"]
    own = (left % 2 == 1) & (left >= 30)
    order = np.concatenate([left[:30], left[own], left[(~own) & (left >= 30)]])
    use = np.concatenate([np.ones(30, bool), np.zeros(int(own.sum()), bool), np.ones(int(((~own) & (left >= 30)).sum()), bool)])
    Qown = np.tile(3.0 * p["qc"], (int(own.sum()), 1, 1))
    p["gp_left"], p["gp_dt"] = left[:30], dt[:30]
    pair = []
    for s in (gp.ChainSolver(gp.LINEAR3), O.Chain(O.LINEAR3)):
        S.apply(p, s)
        s.add_gp_priors_qc(left[own], dt[left[own]], Qown)
        rest = left[(~own) & (left >= 30)]
        s.add_gp_priors(rest, dt[rest])
        s.compile()
        pair.append(s)
    dev, orc = pair
    gn(dev, 2)
    dev.marginals()
    ref = reference(orc, dev, order, dt[order], use=use)
    assert ref[1] == int(use.sum()) == 30 + 45
    check("half own Qc", dev, ref)
    # no prior on the shared Qc at all: n_f = 0, A = 0
    none = gp.ChainSolver(gp.LINEAR3)
    q = dict(p)
    q["gp_left"], q["gp_dt"] = left[:0], dt[:0]
    S.apply(q, none)
    none.add_gp_priors_qc(left, dt, np.tile(Qown[0], (len(left), 1, 1)))
    none.compile()
    gn(none, 1)
    none.marginals()
    A, n_f = none.qc_statistic()
    assert n_f == 0 and np.all(A == 0.0)


# ---------------------------------------------------------------- 3. the contract
def test_stale_and_refused_calls_carry_their_message_and_launch_nothing():
    p = S.linear_chain(50, D=3)
    dev = solver(p)

    def refused(d, pattern):
        d.launch_census()
        before = _census_counts(d)
        with pytest.raises(gp.GpslamHipError, match=pattern):
            d.qc_statistic()
        assert _census_counts(d) == before, pattern

    refused(dev, r"\(-1\).*stale")                  # before marginals
    dev.marginals()
    dev.qc_statistic()
    dev.set_qc(2.0 * np.asarray(p["qc"]))
    refused(dev, r"\(-1\).*stale")
    dev.compile()
    dev.marginals()
    dev.qc_statistic()
    dev.iterate_gn()
    refused(dev, r"\(-1\).*stale")
    refused(solver(S.rot3_bias_ahrs_chain(40)), r"\(-5\).*qc_statistic.*ROT3_BIAS")
    refused(solver(p, precision=1), r"\(-5\).*qc_statistic.*fp32")
    refused(solver(p, force_sharded=True), r"\(-5\).*qc_statistic.*sharded")
    refused(gp.ChainSolver(gp.LINEAR3), r"\(-1\).*stale")


def test_no_interference_and_determinism():
    p = S.add_loop_closures(S.pose3_chain(300), [[10, 150], [40, 220]], seed=4)
    a, b = solver(p), solver(p)
    gn(a, 2)
    gn(b, 2)
    a.marginals()
    before = a.get_marginals()
    first = a.qc_statistic()
    after = a.get_marginals()                       # (still valid: no "stale")
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    second = a.qc_statistic()
    assert np.array_equal(first[0], second[0]) and first[1] == second[1] == 299
    assert np.array_equal(first[0], first[0].T)
    for _ in range(5):
        ra, sa = a.iterate_gn()
        rb, sb = b.iterate_gn()
        assert (ra, sa.error_before, sa.error_after, sa.delta_inf_norm) == (rb, sb.error_before, sb.error_after, sb.delta_inf_norm)
    a.marginals()
    a.qc_statistic()
    a.run_gn(3)
    b.run_gn(3)
    for x, y in zip(a.get_states(), b.get_states()):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------- 4. learning
def test_learn_qc_raises_the_evidence_step_by_step(linear_problem):
    """ten EM steps from 10 Qc_true on the problem of the evidence tests: log Z never falls (within the evidence's own bound), and
    every step is the model's step from the same Qc"""
    pr, thetas, curve = linear_problem
    dev = _linear_solver(pr, 1.0)
    z = np.zeros((pr["N"], pr["d"]))
    out = EV.learn_qc(dev, 10.0 * pr["Qc0"], z, z, params=dev.default_params(max_iterations=5), steps=10)
    assert len(out) == 10 and np.array_equal(out[0][0], 10.0 * pr["Qc0"])
    tols = []
    for k, (Qc, logz, iters) in enumerate(out):
        ref = QM.textbook(pr, Qc)
        tols.append(evidence_noise(pr, Qc, QM.linear_statistic(pr, Qc)[2]))      # _evidence_tol's rule at this Qc
        print("step %d: log Z %.10g, textbook %.10g, off by %.3g of %.3g, %d iterations" % (k, logz, ref, abs(logz - ref), tols[k], iters))
        assert abs(logz - ref) <= tols[k] and iters >= 1
        if k:
            assert logz >= out[k - 1][1] - (tols[k] + tols[k - 1])
            # the model's step from the Qc the device was at: Qc+ = A / (2 n_f), A within the bound of the statistic
            A, n_f, H, cov_scale, err_scale = QM.linear_statistic(pr, out[k - 1][0], scales=True)
            bound = (tol_of(H) * cov_scale + REL * (err_scale + np.abs(A))) / (2.0 * n_f)
            assert np.all(np.abs(Qc - QM.em_update(A, n_f)) <= bound), (np.abs(Qc - QM.em_update(A, n_f)) / bound).max()
    assert out[-1][1] > out[0][1] + 1.0


def test_learn_qc_settles_on_the_models_fixed_point():
    """Measurements of every state (the sparser problem needs thousands of EM steps): from 10 Qc_true learn_qc runs until
    |Qc+ - Qc| <= 1e-9 |Qc|; there the derivative of the textbook evidence -- the model's G at the device's Qc, which the model test
    holds to finite differences -- is within that test's finite-difference bound of zero, entry by entry, and so is the textbook
    curve's own difference quotient"""
    pr = EM.linear_gp_problem(N=40, d=3, dt=0.1, theta=1.0, every=1, seed=0)
    dev = _linear_solver(pr, 1.0)
    z = np.zeros((pr["N"], pr["d"]))
    out = EV.learn_qc(dev, 10.0 * pr["Qc0"], z, z, params=dev.default_params(max_iterations=3), steps=1000, rtol=1e-9)
    assert len(out) < 1000
    Qc = out[-1][0]
    star = QM.em_fixed_point(pr, Qc, 2000, rtol=1e-12)[-1]
    A, n_f, H = QM.linear_statistic(pr, Qc)
    G = QM.gradient(Qc, A, n_f)
    noise = evidence_noise(pr, Qc, H)
    print("%d steps; |Qc - model's fixed point| / |Qc| %.3g; |G| %.3g" % (len(out), np.linalg.norm(Qc - star) / np.linalg.norm(star), np.abs(G).max()))
    for dW in directions(3):
        f1, f2 = fd_pair(pr, np.linalg.inv(Qc), dW)
        bound = 2.0 * abs(f1 - f2) + noise / H_STEP
        assert abs(float(np.sum(G * dW))) <= bound and abs(f2) <= bound, (dW, G, f2, bound)
    # (the evidence's bound at the two ends of the path; kappa of H moves monotonically with the scale of Qc in between)
    tol = 2.0 * max(noise, evidence_noise(pr, out[0][0], QM.linear_statistic(pr, out[0][0])[2]))
    zs = [o[1] for o in out]
    assert all(zs[k] >= zs[k - 1] - tol for k in range(1, len(zs)))


def test_learn_qc_scale_only_beats_the_sweeps_best_grid_point(linear_problem):
    pr, thetas, curve = linear_problem
    dev = _linear_solver(pr, 1.0)
    z = np.zeros((pr["N"], pr["d"]))
    par = dev.default_params(max_iterations=5)
    out5, _ = EV.qc_scale_sweep(dev, pr["Qc0"], thetas, z, z, params=par)
    best = float(out5[:, 0].max())
    out = EV.learn_qc(dev, 10.0 * pr["Qc0"], z, z, params=par, steps=200, rtol=1e-6, scale_only=True)
    theta = out[-1][0][0, 0] / pr["Qc0"][0, 0]
    assert np.abs(out[-1][0] - theta * pr["Qc0"]).max() <= 1e-13 * theta * np.abs(pr["Qc0"]).max()
    tol = _evidence_tol(pr, theta, out5[int(np.argmax(out5[:, 0])), 1])
    print("%d steps: theta %.6g, log Z %.10g; the grid's best %.10g at theta %.3g" % (len(out), theta, out[-1][1], best, thetas[int(np.argmax(out5[:, 0]))]))
    assert len(out) < 200
    assert out[-1][1] >= best - 2 * tol
    assert all(out[k][1] >= out[k - 1][1] - 2 * tol for k in range(1, len(out)))
