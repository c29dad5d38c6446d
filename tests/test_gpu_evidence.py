"""log det H and the Laplace log-evidence on the device (include/gpslam_hip_evidence.h, gpslam_amd/csrc/evidence.hip) against numpy.

Reference of every device number: numpy on the oracle's dense H at the device's states (np.linalg.slogdet, itself held to the bound
against the pivots of np.linalg.cholesky: evidence_model.reference_logdet).  Tolerance of a log-determinant: from
d log det H = tr(H^-1 dH) the absolute error is at most n * 100 EPS kappa, kappa the condition number of the Jacobi-scaled H as
test_gpu_marginals.tol_of computes it (capped at 1e9), floored at n * 1e-13 (evidence_model.logdet_tol).  The one chain too long for a
dense reference (4097 states) takes the plain block recursion and a kappa from power iterations (banded_reference_logdet).  Scalars of
host arithmetic (the normaliser, the combination, the cost) are held at 1e-11 relative, the bound of the dogleg's scalars."""
import os

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import evidence as EV
from gpslam_amd import plaza
from gpslam_amd import synthetic as S
from oracle import oracle as O
import evidence_model as EM
import fixed_lag_mix_model as FM
import marginals_mix_model as MX
from test_gpu_marginals import CHAINS, oracle_H, dense_H, solver, gn, _anchored_range_chain, _free_bytes
from test_gpu_vw import build_vw_pair
from test_gpu_closure_passes import _pairs, _device, _info
from test_gpu_closure import _anchored, _strip_landmarks
from test_gpu_marginals_mix import device, here
from test_gpu_dogleg import device as hooked_device
import dogleg_model as DM

pytestmark = pytest.mark.gpu
REL = 1e-11


def check_logdet(what, dev, H, parts=None):
    """log_determinant of dev against slogdet(H); parts: the reference's three, or None.  Returns (device value, reference, bound)."""
    ref, tol = EM.reference_logdet(H)
    got, p3 = dev.log_determinant(parts=True)
    print("%s: log det H %.12g, reference %.12g, off by %.3g of %.3g; parts %s" % (what, got, ref, abs(got - ref), tol, p3))
    assert got == (p3[0] + p3[1]) + p3[2]
    assert abs(got - ref) <= tol, (what, got, ref, tol)
    if parts is not None:
        for k in range(3):
            assert abs(p3[k] - parts[k]) <= tol, (what, k, p3, parts, tol)
    return got, ref, tol


def split_parts(H, n, Hxx0=None):
    """(log det A, log det(I + U Z), log det S) of the dense H with n state coordinates; Hxx0: the state block without the
    closures (None: there are none)"""
    Hxx = H[:n, :n]
    A = Hxx if Hxx0 is None else Hxx0
    ld_a = float(np.linalg.slogdet(A)[1])
    ld_x = float(np.linalg.slogdet(Hxx)[1])
    ld_s = float(np.linalg.slogdet(H[n:, n:] - H[n:, :n] @ np.linalg.solve(Hxx, H[:n, n:]))[1]) if H.shape[0] > n else 0.0
    return ld_a, ld_x - ld_a, ld_s


# ---------------------------------------------------------------- 1. chains
@pytest.mark.parametrize("name", sorted(k for k in CHAINS if k != "rot3_bias") + ["pose3_vw"])
def test_chain_log_determinant_every_manifold(name):
    if name == "pose3_vw":
        orc, dev, _, _ = build_vw_pair(130, 3)
    else:
        p = CHAINS[name]()
        dev = solver(p)
        orc = S.apply(p, O.Chain(p["kind"]))
    gn(dev, 3)
    H = oracle_H(orc, dev)
    check_logdet(name, dev, H)
    assert dev.log_determinant(parts=True)[1][1:] == (0.0, 0.0)


@pytest.mark.parametrize("N", [1, 2, 15, 16, 17, 33, 257, 4097])
def test_linear2_lengths_across_the_partition(N):
    """one, two, three and four levels; chunk ends; a trailing chunk of one state (17, 33, 257, 4097); a level whose last chunk has
    no right separator"""
    p = S.linear_chain(N, D=2, every=3)
    dev = solver(p)
    gn(dev, 1)
    D, O_, _, _ = dev.normal_equations()
    if N <= 257:
        check_logdet("linear2 N = %d" % N, dev, dense_H(D, O_))
        return
    ref, tol = EM.banded_reference_logdet(D, O_)
    got = dev.log_determinant()
    print("linear2 N = %d: log det H %.12g, banded reference %.12g, off by %.3g of %.3g" % (N, got, ref, abs(got - ref), tol))
    assert abs(got - ref) <= tol
    model, levels = EM.chain_logdet(D, O_)
    assert levels == 4 and abs(got - model) <= tol


def test_pose3_chain_of_257_states():
    p = S.pose3_chain(257)
    dev = solver(p)
    orc = S.apply(p, O.Chain(O.POSE3))
    gn(dev, 2)
    check_logdet("pose3 N = 257", dev, oracle_H(orc, dev))


# ---------------------------------------------------------------- 2. landmarks and closures
def test_landmarks_on_the_dense_border_all_three_parts():
    p = _anchored_range_chain(60)
    dev = solver(p, landmark_dim=2)
    gn(dev, 3)
    orc = S.apply(p, O.Chain(O.POSE2, landmark_dim=2))
    H = oracle_H(orc, dev)
    n = dev.N * dev.b
    assert H.shape[0] == n + 16
    check_logdet("60 states, 8 landmarks", dev, H, split_parts(H, n))


def _pose2_base():
    """150 states: kappa of the Jacobi-scaled H is 5e7 without closures (the 300 states of test_gpu_closure_passes: 8.6e8, next to the cap)"""
    return _anchored(_strip_landmarks(S.pose2_range_chain(150, seed=9)))


def _closure_case(name):
    if name == "pose2_9":       # closures at both chain ends
        return S.add_loop_closures(_pose2_base(), [[0, 149], [149, 3], [1, 75]] + _pairs(150, 6, 21), seed=5), O.POSE2, None, (9, 9, 1)
    if name == "pose3_4":
        return S.add_loop_closures(S.pose3_chain(200, seed=2), [[0, 199], [199, 40], [60, 10], [100, 150]], seed=4), O.POSE3, None, (4, 4, 1)
    if name == "pose2_12":
        return S.add_loop_closures(_pose2_base(), _pairs(150, 12, 21), seed=5), O.POSE2, 32, (12, 9, 2)
    if name == "pose2_40":
        return S.add_loop_closures(_pose2_base(), _pairs(150, 40, 21), seed=5), O.POSE2, 32, (40, 9, 5)
    if name == "pose3_20":
        return S.add_loop_closures(S.pose3_chain(200, seed=2), _pairs(200, 20, 31), seed=8), O.POSE3, 32, (20, 4, 5)
    assert name == "pose2_10_lm8"     # 8 landmark columns leave room for 6 closures per pass
    return S.add_loop_closures(_anchored(S.pose2_range_chain(200, L=4, seed=3)), _pairs(200, 10, 51), seed=7), O.POSE2, 32, (10, 6, 2)


@pytest.mark.parametrize("name", ["pose2_9", "pose3_4", "pose2_12", "pose2_40", "pose3_20", "pose2_10_lm8"])
def test_loop_closures_in_one_pass_and_in_column_passes(name):
    """one pass: k_ev_core forms U Z from the records and the solution's closure columns; column passes: from clo.W, with no kept Z
    (marginals_keep_closure_columns is never called)"""
    p, kind, max_passes, info = _closure_case(name)
    ld = 2 if "landmarks" in p else 0
    dev = _device(p, max_passes)
    _info(dev, *info)
    orc = S.apply(p, O.Chain(kind, landmark_dim=ld))
    gn(dev, 2)
    H = oracle_H(orc, dev, p)
    n = dev.N * dev.b
    bare = S.apply({k: v for k, v in p.items() if not k.startswith("closure_")}, O.Chain(kind, landmark_dim=ld))
    H0 = oracle_H(bare, dev)[:n, :n]         # the chain part A: the graph without its closures, at the same states
    check_logdet(name, dev, H, split_parts(H, n, H0))


# ---------------------------------------------------------------- 3. robust losses, state and border Gaussians
def test_robust_graph_matches_the_reweighted_H_and_has_no_evidence():
    p = MX.graph("se2", robust=True)
    dev = device(p)
    gn(dev, 2)
    ph = here(p, dev)
    h = device(FM.plain(ph))
    rw = FM.robust_weights(ph, FM.plain_errors(ph, h))
    h.close()
    H = MX.H_of(FM.reweighted(ph, {pre: w for pre, (r, w) in rw.items()}))
    check_logdet("robust se2", dev, H)
    before = _census_counts(dev)
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*log_evidence.*robust loss"):
        dev.log_evidence()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*log_noise_normaliser.*factor \d+ carries a robust loss"):
        dev.log_noise_normaliser()
    assert _census_counts(dev) == before


@pytest.mark.parametrize("name,onto", [("se2", True), ("se3_vw", False)])
def test_state_and_border_gaussians_match_the_augmented_H_and_have_no_evidence(name, onto):
    p = MX.graph(name)
    k = 5
    dev = device(p, onto)
    dev.marginalize_head(k)
    dev.compile()
    dev.iterate_gn()
    Lam = dev.get_head_prior_border()[1] if onto else dev.get_head_prior()[2]
    H = MX.H_of(here(FM.window(p, k, FM.NS[name]), dev), lambdas=[(0, Lam)])
    check_logdet("%s behind marginalize_head(%d)" % (name, k), dev, H)
    before = _census_counts(dev)
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*log_evidence.*%s Gaussian 0" % ("border" if onto else "state")):
        dev.log_evidence()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*log_noise_normaliser.*%s Gaussian 0" % ("border" if onto else "state")):
        dev.log_noise_normaliser()
    assert _census_counts(dev) == before


# ---------------------------------------------------------------- 4. the contract
def _census_counts(dev):
    return {k: v for k, v in dev.launch_census(reset=False).items()}


def test_refusals_carry_their_message_and_launch_nothing():
    p = S.linear_chain(50, D=3)
    cases = [
        (lambda: solver(p, precision=1), r"fp32"),
        (lambda: solver(_anchored_range_chain(60), landmark_dim=2, force_segmented=True), r"segmented"),
        (lambda: solver(p, force_sharded=True), r"sharded"),
        (lambda: solver(S.rot3_bias_ahrs_chain(40)), r"ROT3_BIAS"),
        # a split piece on one card, as tests/test_gpu_dogleg.py makes it: segmented, rank 0 of 2
        (lambda: hooked_device(DM.graph("se2", True, 60), lambda s, q: s.fs_set_split(0, 2), force_segmented=True), r"split pieces"),
    ]
    for make, word in cases:
        dev = make()
        dev.launch_census()
        before = _census_counts(dev)
        with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*log_determinant.*" + word):
            dev.log_determinant()
        with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*log_evidence.*" + word):
            dev.log_evidence()
        assert _census_counts(dev) == before, word
    seg = solver(_anchored_range_chain(60), landmark_dim=2, force_segmented=True)
    seg.marginals_on_segments()
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*segmented"):
        seg.log_determinant()
    ahrs = solver(S.rot3_bias_ahrs_chain(40))
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*ROT3_BIAS"):
        ahrs.log_noise_normaliser()
    raw = gp.ChainSolver(gp.LINEAR3)
    with pytest.raises(gp.GpslamHipError, match=r"\(-4\)"):
        raw.log_determinant()


def test_unanchored_chain_is_not_spd():
    q = dict(S.linear_chain(50, D=3))
    for k in ("prior_idx", "prior_pose", "prior_sig", "vprior_idx", "vprior", "vprior_sig"):
        q.pop(k)
    with pytest.raises(gp.GpslamHipError, match=r"\(-3\).*log_determinant: (non-positive pivot|a pivot of the chain's elimination is below 2\^-36)"):
        solver(q).log_determinant()


def test_a_chain_next_to_the_condition_cap_clears_the_pivot_floor():
    """300 anchored SE(2) states, kappa of the Jacobi-scaled H about 8.6e8 of the 1e9 the tests admit: every pivot stays above
    2^-36 of its diagonal entry (no GPSLAM_E_NOT_SPD) and the number is within the bound"""
    p = _anchored(_strip_landmarks(S.pose2_range_chain(300, seed=9)))
    dev = solver(p)
    orc = S.apply(p, O.Chain(O.POSE2))
    gn(dev, 2)
    H = oracle_H(orc, dev)
    s = np.sqrt(np.diag(H))
    kappa = np.linalg.cond(H / np.outer(s, s))
    print("kappa %.3g" % kappa)
    assert 5e8 <= kappa <= 1e9
    check_logdet("pose2, 300 states", dev, H)


def test_reruns_are_bit_identical_and_the_handle_goes_on_as_its_twin():
    p = S.add_loop_closures(S.pose3_chain(300), [[10, 150], [40, 220]], seed=4)
    a, b = solver(p), solver(p)
    gn(a, 2)
    gn(b, 2)
    a.marginals()
    a.get_marginals()
    first = a.log_determinant(parts=True)
    with pytest.raises(gp.GpslamHipError, match="stale"):
        a.get_marginals()
    assert a.log_determinant(parts=True) == first
    ev = a.log_evidence()
    assert a.log_evidence() == ev and ev[2] == first[0]
    for _ in range(10):
        ra, sa = a.iterate_gn()
        rb, sb = b.iterate_gn()
        assert (ra, sa.error_before, sa.error_after, sa.delta_inf_norm) == (rb, sb.error_before, sb.error_after, sb.delta_inf_norm)
    for x, y in zip(a.get_states(), b.get_states()):
        assert np.array_equal(x, y)
    a.log_determinant()
    a.run_gn(3)
    b.run_gn(3)
    for x, y in zip(a.get_states(), b.get_states()):
        assert np.array_equal(x, y)


def test_destroy_frees_the_device_memory():
    """A handle's whole life, five times over, as test_gpu_marginals.test_destroy_frees_the_device_memory: a condition on gross leaks"""
    N = 20000
    p = S.pose3_chain(N)

    def cycle():
        dev = solver(p)
        dev.log_determinant()
        inside = _free_bytes()
        dev.close()
        return inside

    cycle()
    free_warm = _free_bytes()
    footprint = free_warm - cycle()
    for _ in range(4):
        cycle()
    lost = free_warm - _free_bytes()
    print("footprint %d bytes, lost after five cycles %d bytes" % (footprint, lost))
    assert footprint >= 3 * 144 * 8 * (N // 16)       # the separators' slabs of level 1 alone
    assert lost < footprint / 2


# ---------------------------------------------------------------- 5. the evidence proper
@pytest.fixture(scope="module")
def linear_problem():
    pr = EM.linear_gp_problem(N=40, d=3, dt=0.1, theta=1.0, every=4, seed=2)
    thetas = 10.0 ** np.arange(-2.0, 2.01, 0.5)
    curve = np.array([EM.gp_marginal_loglik(pr["m0"], pr["P0"], pr["dts"], t * pr["Qc0"], pr["meas_idx"], pr["y"], pr["sig"]) for t in thetas])
    return pr, thetas, curve


def _linear_solver(pr, theta):
    N, d = pr["N"], pr["d"]
    dev = gp.ChainSolver(gp.LINEAR3)
    dev.set_qc(theta * pr["Qc0"])
    dev.set_states(np.zeros((N, d)), np.zeros((N, d)))
    dev.add_gp_priors(np.arange(N - 1, dtype=np.int32), pr["dts"])
    dev.add_pose_priors(np.array([0], dtype=np.int32), pr["m0"][None, :d], pr["sp"][None])
    dev.add_vel_priors(np.array([0], dtype=np.int32), pr["m0"][None, d:], pr["sv"][None])
    dev.add_pose_priors(pr["meas_idx"], pr["y"], pr["sig"])
    dev.compile()
    return dev


def _evidence_tol(pr, theta, cost):
    """the log-det bound of this graph's H (log Z takes half of log det H) plus 1e-11 of the cost"""
    return 0.5 * EM.logdet_tol(_linear_H(pr, theta)) + REL * abs(cost)


def _linear_H(pr, theta):
    N, d = pr["N"], pr["d"]
    orc = O.Chain(O.LINEAR3)
    orc.set_qc(theta * pr["Qc0"])
    orc.set_states(np.zeros((N, d)), np.zeros((N, d)))
    orc.add_gp_priors(np.arange(N - 1, dtype=np.int32), pr["dts"])
    orc.add_pose_priors(np.array([0], dtype=np.int32), pr["m0"][None, :d], pr["sp"][None])
    orc.add_vel_priors(np.array([0], dtype=np.int32), pr["m0"][None, d:], pr["sv"][None])
    orc.add_pose_priors(pr["meas_idx"], pr["y"], pr["sig"])
    orc.compile()
    D, O_, _, _, _, _ = orc.normal_equations()
    return dense_H(D, O_)


def test_log_evidence_of_a_linear_chain_is_the_textbook_marginal_likelihood(linear_problem):
    """LINEAR3, 40 states, every factor linear: Laplace is exact, and log Z = log N(y; C m, C K C^T + R) with K from propagating
    Phi(dt), Q(dt) from the prior on state 0 -- no J, no H on the reference side"""
    pr, thetas, curve = linear_problem
    dev = _linear_solver(pr, 1.0)
    gn(dev, 2)
    logZ, cost, logdet, lognorm, mn = dev.log_evidence()
    ref = float(curve[list(thetas).index(1.0)])
    tol = _evidence_tol(pr, 1.0, cost)
    print("log Z %.12g, textbook %.12g, off by %.3g of %.3g (cost %.6g, log det H %.6g, lognorm %.6g, m - n %d)" % (logZ, ref, abs(logZ - ref), tol, cost, logdet, lognorm, mn))
    assert mn == pr["y"].size == 30
    assert abs(logZ - ref) <= tol
    # the parts, each against its own reference
    mZ, mcost, mlogdet, mlognorm, _ = EM.linear_gp_graph_logZ(pr, 1.0)
    assert abs(lognorm - mlognorm) <= REL * abs(mlognorm)
    assert dev.log_noise_normaliser() == (lognorm, 270, 240)
    assert cost == dev.error()
    print("cost %.15g, the dense model's %.15g" % (cost, mcost))
    assert abs(cost - mcost) <= REL * mcost
    assert logZ == gp.evidence_combine(cost, logdet, lognorm, 270, 240)
    check_logdet("the linear chain", dev, _linear_H(pr, 1.0))


def test_qc_scale_sweep_follows_the_textbook_curve(linear_problem):
    pr, thetas, curve = linear_problem
    dev = _linear_solver(pr, 1.0)
    z = np.zeros((pr["N"], pr["d"]))
    out5, iters = EV.qc_scale_sweep(dev, pr["Qc0"], thetas, z, z, params=dev.default_params(max_iterations=5))
    for k, t in enumerate(thetas):
        tol = _evidence_tol(pr, t, out5[k, 1])
        print("theta %8.3g: log Z %.10g, textbook %.10g, off by %.3g of %.3g, %d iterations" % (t, out5[k, 0], curve[k], abs(out5[k, 0] - curve[k]), tol, iters[k]))
        assert abs(out5[k, 0] - curve[k]) <= tol
    assert int(np.argmax(out5[:, 0])) == int(np.argmax(curve))
    assert np.all(iters >= 1)


def _plaza_lognorm(p, theta):
    """(sum_f log|det R_f|, m, n) of the Plaza graph in numpy from its description: priors, odometry, ranges, GP priors at theta * qc"""
    N, L = p["N"], len(p["landmarks"])
    total = -float(np.sum(np.log(p["prior_sig"]))) - float(np.sum(np.log(p["lprior_sig"]))) - float(np.sum(np.log(p["between_sig"])))
    total -= float(np.sum(np.log(p["range_sigma"])))
    total += float(sum(EM.gp_log_normaliser(theta * p["qc"], dt) for dt in p["gp_dt"]))
    m = p["prior_sig"].size + p["lprior_sig"].size + p["between_sig"].size + p["range_sigma"].size + 6 * len(p["gp_dt"])
    return total, m, 6 * N + 2 * L


@pytest.mark.parametrize("theta", [0.3, 1.0, 10.0])
def test_plaza2_evidence_at_three_scales(theta):
    """Plaza2 with its 4 landmarks, one scale of Qc per case (kappa of the oracle's Jacobi-scaled chain part grows as Qc shrinks: 2.5e7
    at 10, 1.6e8 at 1, 1.6e9 at 0.1, which is past the cap of 1e9 every reference here keeps, so the smallest scale is 0.3): qc_scale_sweep optimises, and log Z is held to the formula over the
    oracle's cost and H at the device's optimum (the chain part by the plain block recursion, the landmarks' Schur complement dense:
    the graph has no closures) and a normaliser summed in numpy from the graph's description"""
    data = plaza.load(os.path.join(os.path.dirname(__file__), "golden", "plaza2.npz"))
    p = plaza.build_problem(data)
    dev = plaza.apply(p, gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER, landmark_dim=2))
    out5, iters = EV.qc_scale_sweep(dev, p["qc"], [theta], p["pose"], p["vel"], p["landmarks"],
                                    params=dev.default_params(use_lm=1, max_iterations=30))
    logZ, dcost, dlogdet, dlognorm, mn = out5[0]
    orc = plaza.apply(dict(p, qc=theta * p["qc"]), O.Chain(O.POSE2, chart=O.CHART_FIRST_ORDER, landmark_dim=2))
    pose, vel = dev.get_states()
    orc.set_states(pose, vel)
    orc.set_landmarks(dev.get_landmarks())
    D, O_, _, B, HLL, _ = orc.normal_equations()
    ld_a, tol = EM.banded_reference_logdet(D, O_)
    N, b, nl = B.shape
    Bf = B.reshape(N * b, nl)
    X = _banded_solve(D, O_, Bf)
    ld_s = float(np.linalg.slogdet(HLL - Bf.T @ X)[1])
    cost = orc.error()
    lognorm, m, n = _plaza_lognorm(p, theta)
    ref = EM.combine(cost, ld_a + ld_s, lognorm, m, n)
    bound = 0.5 * tol + REL * abs(cost)
    print("Plaza2 (%d states) at theta %g: %d iterations, log Z %.12g, reference %.12g, off by %.3g of %.3g; cost %.15g, oracle's %.15g; "
          "lognorm %.15g, numpy's %.15g; log det H off by %.3g of %.3g"
          % (N, theta, iters[0], logZ, ref, abs(logZ - ref), bound, dcost, cost, dlognorm, lognorm, abs(dlogdet - (ld_a + ld_s)), tol))
    assert dev.log_noise_normaliser()[1:] == (m, n) and mn == m - n and n == N * b + nl
    assert abs(dlognorm - lognorm) <= REL * abs(lognorm)
    assert abs(dcost - cost) <= REL * cost
    assert abs(dlogdet - (ld_a + ld_s)) <= tol
    assert abs(logZ - ref) <= bound


# ---------------------------------------------------------------- 6. the normaliser on every noise model
def test_noise_normaliser_on_every_kind_of_noise_model():
    """A small planar graph with landmarks ([x y theta] vector states: the manifold that has bearing-range factors; ranges and bearings
    are nonlinear in it) that carries every noise model ev_lognorm walks: GP priors with the handle's Qc and, through
    add_gp_priors_qc in two calls, with two distinct full Qc in mixed order (the slots of gp_Qtab), pose and velocity priors, between
    factors, landmark priors, ranges of which two took a 1 x 1 covariance, bearing-range factors of which two took a full 2 x 2
    covariance, one loop closure.  The sum, rows and variables against numpy at 1e-11."""
    rng = np.random.default_rng(17)
    N, L, d = 12, 3, 3

    def spd(n):
        G = rng.standard_normal((n, n))
        return G @ G.T / n + 0.3 * np.eye(n)
    Qh, Qa, Qb = spd(3), spd(3), spd(3)
    pose = np.stack([0.3 * np.arange(N), 0.05 * np.sin(np.arange(N)), 0.02 * np.arange(N)], -1)
    lmk = np.array([[1.0, 2.0], [2.5, -1.5], [4.0, 1.0]])
    dev = gp.ChainSolver(gp.LINEAR3, landmark_dim=2)
    dev.set_qc(Qh)
    dev.set_states(pose, np.tile([1.2, 0.0, 0.08], (N, 1)))
    dev.set_landmarks(lmk)
    dts = rng.uniform(0.05, 0.4, N - 1)
    total = 0.0
    dev.add_gp_priors(np.arange(0, 3, dtype=np.int32), dts[:3])
    qcs = [Qh] * 3
    for lo, hi, pick in ((3, 8, [Qa, Qb, Qa, Qb, Qa]), (8, 11, [Qb, Qa, Qb])):
        dev.add_gp_priors_qc(np.arange(lo, hi, dtype=np.int32), dts[lo:hi], np.stack(pick))
        qcs += pick
    total += sum(EM.gp_log_normaliser(Q, dt) for Q, dt in zip(qcs, dts))
    rows = 2 * d * (N - 1)

    def diag(sig):
        nonlocal total, rows
        total -= float(np.sum(np.log(sig)))
        rows += sig.size
        return sig
    dev.add_pose_priors(np.array([0], dtype=np.int32), pose[:1], diag(rng.uniform(0.01, 0.2, (1, 3))))
    dev.add_vel_priors(np.array([0], dtype=np.int32), np.array([[1.2, 0.0, 0.08]]), diag(rng.uniform(0.1, 1.0, (1, 3))))
    rel = np.tile([0.3, 0.0, 0.02], (N - 1, 1))
    dev.add_between(np.arange(N - 1, dtype=np.int32), rel, diag(rng.uniform(0.005, 0.05, (N - 1, 3))))
    dev.add_landmark_priors(np.array([0, 2], dtype=np.int32), lmk[[0, 2]], diag(rng.uniform(0.2, 2.0, (2, 2))))
    ri, rl = np.array([1, 3, 5, 7, 9], dtype=np.int32), np.array([0, 1, 2, 0, 1], dtype=np.int32)
    rsig = rng.uniform(0.1, 0.6, 5)
    dev.add_range(ri, rl, np.linalg.norm(lmk[rl] - pose[ri, :2], axis=1), rsig)
    rcov = rng.uniform(0.01, 0.5, (2, 1, 1))
    dev.set_meas_covariance(gp.chain.MEAS_RANGE, rcov)                  # the last two ranges: a 1 x 1 Gaussian is a sigma
    total += -float(np.sum(np.log(rsig[:3]))) - 0.5 * float(np.sum(np.log(rcov)))
    rows += 5
    bi, bl = np.array([2, 4, 6, 8], dtype=np.int32), np.array([2, 1, 0, 2], dtype=np.int32)
    dl = lmk[bl] - pose[bi, :2]
    bsig = rng.uniform(0.02, 0.3, (4, 2))
    dev.add_bearing_range(bi, bl, np.arctan2(dl[:, 1], dl[:, 0]), np.linalg.norm(dl, axis=1), bsig)
    bcov = np.stack([spd(2) * 0.05, spd(2) * 0.2])
    dev.set_meas_covariance(gp.chain.MEAS_BEARING_RANGE, bcov)          # the last two: full 2 x 2 covariances beside two diagonal models
    total += -float(np.sum(np.log(bsig[:2]))) - 0.5 * float(sum(np.linalg.slogdet(c)[1] for c in bcov))
    rows += 8
    dev.add_between_pairs([1], [10], pose[10:11] - pose[1:2], diag(rng.uniform(0.02, 0.1, (1, 3))))
    got, m, n = dev.log_noise_normaliser()                               # (host arithmetic over the stored graph: before compile())
    print("lognorm %.15g, numpy %.15g, off by %.3g of %.3g; rows %d, variables %d" % (got, total, abs(got - total), REL * abs(total), m, n))
    assert (m, n) == (rows, 2 * d * N + 2 * L) == (125, 78)
    assert abs(got - total) <= REL * abs(total)
    dev.compile()
    out5 = dev.log_evidence()
    assert out5[3] == got and out5[4] == rows - n
    assert out5[0] == gp.evidence_combine(out5[1], out5[2], got, m, n)


def _banded_solve(D, O_, R):
    """A^-1 R for the block-tridiagonal A = (D, O_) by the plain block recursion"""
    N, b = D.shape[0], D.shape[1]
    Y = R.reshape(N, b, -1).copy()
    P = np.zeros_like(D)
    P[0] = D[0]
    for i in range(N - 1):
        G = np.linalg.solve(P[i], O_[i].T).T
        P[i + 1] = D[i + 1] - G @ O_[i].T
        Y[i + 1] -= G @ Y[i]
    X = np.zeros_like(Y)
    X[N - 1] = np.linalg.solve(P[N - 1], Y[N - 1])
    for i in range(N - 2, -1, -1):
        X[i] = np.linalg.solve(P[i], Y[i] - O_[i].T @ X[i + 1])
    return X.reshape(N * b, -1)
