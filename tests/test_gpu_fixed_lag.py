"""Fixed-lag smoothing on the device (gpslam_amd/csrc/fixedlag.hip) against the oracle's arrays and the numpy model of
tests/fixed_lag_model.py: the state Gaussian factor, Lambda / gamma of the marginalised head, one and several Gauss-Newton steps
against the batch problem, a sliding window against the batch solution, and the refusals.

Tolerance of Lambda / gamma (lam_tol): 100 x the largest distance, over the cases of test_lambda_gamma, between the model run in
float64 and in np.longdouble on the oracle's float64 normal equations, relative to max |D_k^left| (gamma: max |g|); asserted to stay
below 1e-10.  The factor 100 covers the device's different summation order over k b^2 terms."""
import functools

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import synthetic as S
from oracle import oracle as O
from helpers import pose_close
from test_gpu_parity import random_chain, states_close
import fixed_lag_model as FL

pytestmark = pytest.mark.gpu
KINDS = {"linear2": O.LINEAR2, "linear3": O.LINEAR3, "pose2": O.POSE2, "rot3": O.ROT3, "pose3": O.POSE3}


def identity(kind):
    if kind == O.POSE3:
        return O.pose3((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    if kind == O.ROT3:
        return O.rot3_ypr(0.0, 0.0, 0.0)
    return np.zeros(O.POSE_DIM[kind])


@functools.lru_cache(maxsize=None)
def problem(name, N, k=None, seed=3):
    """A GP chain with a prior on state 0, odometry and a velocity prior; with k, also what must and must not enter the head's prior:
    an interpolated GPS (pose3) / attitude (rot3) factor on (k - 1, k) -- in the head --, one on (k, k + 1) and a pose prior on
    state k -- not in it."""
    kind = KINDS[name]
    d = O.TANGENT_DIM[kind]
    c = random_chain(kind, N, seed)
    rng = np.random.default_rng(seed + 100)
    i = np.arange(N - 1, dtype=np.int32)
    p = dict(kind=kind, N=N, qc=np.diag(0.5 + rng.random(d)), pose=c["pose"], vel=c["vel"], gp_left=i, gp_dt=c["dt"],
             prior_idx=np.array([0], dtype=np.int32), prior_pose=c["truth_pose"][:1].copy(), prior_sig=np.full((1, d), 0.05),
             vprior_idx=np.array([0], dtype=np.int32), vprior=c["truth_vel"][:1].copy(), vprior_sig=np.full((1, d), 0.1),
             between_left=i, between_meas=np.stack([O.retract(kind, identity(kind), c["dt"][j] * c["truth_vel"][j]) for j in i]),
             between_sig=np.full((N - 1, d), 0.05))
    if k is not None:
        p["prior_idx"] = np.array([0, k], dtype=np.int32)
        p["prior_pose"] = c["truth_pose"][[0, k]].copy()
        p["prior_sig"] = np.full((2, d), 0.05)
        left = np.array([j for j in (k - 1, k) if j + 1 < N], dtype=np.int32)
        M = len(left)
        if kind == O.POSE3:
            p.update(gps_left=left, gps_meas=c["truth_pose"][left, 9:12] + 0.05 * rng.standard_normal((M, 3)), gps_sigma=np.full((M, 3), 0.1),
                     gps_dt=c["dt"][left], gps_tau=0.4 * c["dt"][left])
        if kind == O.ROT3:
            R = c["truth_pose"][left].reshape(M, 3, 3)
            nz = R[:, :, 2] + 0.05 * rng.standard_normal((M, 3))
            p.update(att_left=left, att_nz=nz / np.linalg.norm(nz, axis=1, keepdims=True), att_bref=np.tile([0.0, 0.0, 1.0], (M, 1)),
                     att_sigma=np.full((M, 2), 0.1), att_dt=c["dt"][left], att_tau=0.4 * c["dt"][left])
    return p


def solver(p, **kw):
    return S.apply(p, gp.ChainSolver(p["kind"], **kw))


def head_reference(p, k, dtype=np.float64):
    head, _ = FL.head_tail(p, k)
    D, Om, g = S.apply(head, O.Chain(p["kind"])).normal_equations()[:3]
    Lam, gam, _ = FL.schur(D, Om, g, k, dtype)
    return Lam, gam, float(np.abs(D[k]).max()), float(np.abs(g).max())


LG_CASES = [(n, k) for n in ("pose2", "rot3", "linear3", "pose3") for k in (1, 2, 5, 11)]


@functools.lru_cache(maxsize=None)
def lam_tol():
    worst = 0.0
    for name, k in LG_CASES:
        p = problem(name, 12, k)
        L0, g0, sD, sg = head_reference(p, k)
        L1, g1, _, _ = head_reference(p, k, np.longdouble)
        worst = max(worst, float(np.abs(L0 - L1).max()) / sD, float(np.abs(g0 - g1).max()) / sg)
    tol = 100.0 * worst
    print("model float64 against longdouble: %.3g relative; tolerance %.3g" % (worst, tol))
    assert 0.0 < tol < 1e-10
    return tol


# ---------------------------------------------------------------- 1. the factor
def factor_chain(name, chart, vw):
    kind = O.POSE3 if name == "pose3_vw" else KINDS[name]
    d, b = O.TANGENT_DIM[kind], 2 * O.TANGENT_DIM[kind]
    c = random_chain(kind, 3, 21)
    rng = np.random.default_rng(8)
    kw = dict(velocity_world=True) if vw else {}
    orc, dev = O.Chain(kind, chart=chart, **kw), gp.ChainSolver(kind, chart=chart, **kw)
    for s in (orc, dev):
        s.set_qc(np.diag(0.5 + np.arange(d) * 0.1))
        s.set_states(c["pose"], c["vel"])
        s.add_gp_priors(np.arange(2), c["dt"])
        s.compile()
    idx = np.array([0, 1, 2], dtype=np.int32)
    lin_p = np.stack([O.retract(kind, c["pose"][i], 0.3 * rng.standard_normal(d), chart) for i in idx])
    lin_v = c["vel"][idx] + 0.3 * rng.standard_normal((3, d))
    A, cc = rng.standard_normal((3, b, b)), rng.standard_normal((3, b))
    return kind, chart, c, orc, dev, idx, lin_p, lin_v, A, cc


@pytest.mark.parametrize("name,chart", [("linear2", 0), ("linear3", 0), ("pose2", 0), ("pose2", 1), ("rot3", 0), ("pose3", 0), ("pose3_vw", 0)])
def test_state_gaussian_rows_and_error(name, chart):
    kind, chart, c, orc, dev, idx, lin_p, lin_v, A, cc = factor_chain(name, chart, name == "pose3_vw")
    b = dev.b
    dev.add_state_gaussians(idx, lin_p, lin_v, A, cc)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-4\)"):
        dev.error()
    dev.compile()
    got = dev.get_state_gaussians()
    for a, e in zip(got, (idx, lin_p, lin_v, A, cc)):
        assert np.array_equal(a, e)
    LR, E, _, _ = dev.get_rows()
    assert LR.shape[0] == 5 * b
    first = [b, 3 * b, 4 * b]      # behind the GP prior's rows of states 0 and 1; state 2 has no other row
    tot = 0.0
    for f in range(3):
        r = FL.residual(kind, chart, lin_p[f], lin_v[f], A[f], cc[f], c["pose"][idx[f]], c["vel"][idx[f]])
        rows = slice(first[f], first[f] + b)
        assert np.abs(LR[rows, :b] - A[f]).max() <= 1e-11
        assert np.all(LR[rows, b:] == 0.0)
        assert np.abs(E[rows] - r).max() <= 1e-11
        tot += 0.5 * float(r @ r)
    ref = orc.error() + tot
    assert abs(dev.error() - ref) <= 1e-11 * ref
    dev.clear_factors()
    assert dev.get_state_gaussians()[0].size == 0


def test_block_diagonal_gaussian_is_pose_prior_plus_velocity_prior():
    p = problem("linear3", 3)
    kind, d = p["kind"], 3
    rng = np.random.default_rng(4)
    sig = 0.05 + rng.random((2, 2 * d))
    at = np.array([0, 2], dtype=np.int32)
    mp, mv = p["pose"][at] + 0.3, p["vel"][at] - 0.2
    a, bdev = solver(p), solver(p)
    a.add_pose_priors(at, mp, sig[:, :d])
    a.add_vel_priors(at, mv, sig[:, d:])
    bdev.add_state_gaussians(at, mp, mv, np.stack([np.diag(1.0 / s) for s in sig]), np.zeros((2, 2 * d)))
    for s in (a, bdev):
        s.compile()
        s.iterate_gn()
    (pa, va), (pb, vb) = a.get_states(), bdev.get_states()
    assert np.abs(pa - pb).max() <= 1e-12 and np.abs(va - vb).max() <= 1e-12


# ---------------------------------------------------------------- 2. Lambda, gamma
@pytest.mark.parametrize("name,k", LG_CASES)
def test_lambda_gamma(name, k):
    tol = lam_tol()
    p = problem(name, 12, k)
    dev = solver(p)
    dev.marginalize_head(k)
    assert dev.N == 12 - k
    pl, vl, Lam, gam = dev.get_head_prior()
    assert np.array_equal(pl, p["pose"][k]) and np.array_equal(vl, p["vel"][k])
    L0, g0, sD, sg = head_reference(p, k)
    eL, eg = float(np.abs(Lam - L0).max()) / sD, float(np.abs(gam - g0).max()) / sg
    print("%s k = %d: device against model %.3g (Lambda), %.3g (gamma) relative; tolerance %.3g" % (name, k, eL, eg, tol))
    assert np.linalg.eigvalsh(0.5 * (L0 + L0.T)).min() > 0.0
    assert eL <= tol and eg <= tol
    idx, _, _, A, c = dev.get_state_gaussians()
    assert list(idx) == [0]
    assert np.abs(A[0].T @ A[0] - 0.5 * (Lam + Lam.T)).max() <= 1e-13 * sD
    assert np.abs(A[0].T @ c[0] + gam).max() <= 1e-11 * sg


# ---------------------------------------------------------------- 3. / 4. one step and several steps equal batch
def check_states(kind, dp, dv, rp, rv, tol=1e-9):
    assert np.abs(dv - rv).max() <= tol
    for a, b in zip(dp, rp):
        assert pose_close(kind, a, b, tol)


@pytest.mark.parametrize("name", ["pose2", "pose3", "rot3"])
@pytest.mark.parametrize("where", ["first", "last"])
def test_one_step_equals_batch_then_tracks_the_model(name, where):
    N = 9
    k = 1 if where == "first" else N - 1
    p = problem(name, N, k)
    kind = p["kind"]
    orc = S.apply(p, O.Chain(kind))
    dev = solver(p)
    dev.marginalize_head(k)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-4\)"):
        dev.iterate_gn()
    dev.compile()
    orc.iterate_gn()
    dev.iterate_gn()
    bp, bv = orc.get_states()
    dp, dv = dev.get_states()
    check_states(kind, dp, dv, bp[k:], bv[k:])
    # several steps: the model's reference iteration on the tail-only oracle chain with the device's prior
    _, tail = FL.head_tail(p, k)
    tail["pose"], tail["vel"] = dp, dv
    ref = S.apply(tail, O.Chain(kind))
    idx, pl, vl, A, c = dev.get_state_gaussians()
    gaussians = [(int(idx[0]), pl[0], vl[0], A[0], c[0])]
    for _ in range(3):
        rp, rv = FL.gn_step(ref, kind, O.CHART_EXPMAP, gaussians)
        dev.iterate_gn()
        dp, dv = dev.get_states()
        check_states(kind, dp, dv, rp, rv)


@pytest.mark.parametrize("name", ["pose2", "pose3"])
def test_optimize_lm_after_marginalisation(name):
    p = problem(name, 9, 3)
    dev = solver(p)
    dev.marginalize_head(3)
    dev.compile()
    g0 = np.abs(dev.normal_equations()[2]).max()
    dev.optimize(dev.default_params(use_lm=1, max_iterations=50, relative_error_tol=1e-14, absolute_error_tol=1e-14))
    assert np.abs(dev.normal_equations()[2]).max() <= 1e-6 * g0


def test_landmarks_seen_from_the_tail_keep_their_indices():
    N, k = 9, 3
    p = dict(problem("pose2", N, k))
    rng = np.random.default_rng(2)
    lm = np.array([[3.0, 1.0], [-2.0, 4.0]])
    at = np.array([3, 4, 6, 8, 5, 7], dtype=np.int32)
    which = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    z = np.linalg.norm(lm[which] - p["pose"][at, :2], axis=1) + 0.05 * rng.standard_normal(6)
    orc, dev = O.Chain(O.POSE2, landmark_dim=2), gp.ChainSolver(O.POSE2, landmark_dim=2)
    for s in (orc, dev):
        S.apply(p, s)
        s.set_landmarks(lm + 0.1)
        s.add_landmark_priors([0, 1], lm, np.full((2, 2), 0.5))
        s.add_range(at, which, z, np.full(6, 0.1))
        s.compile()
    dev.marginalize_head(k)
    dev.compile()
    orc.iterate_gn()
    dev.iterate_gn()
    bp, bv = orc.get_states()
    dp, dv = dev.get_states()
    check_states(O.POSE2, dp, dv, bp[k:], bv[k:])
    assert np.abs(dev.get_landmarks() - orc.get_landmarks()).max() <= 1e-9
    # a head factor that names a landmark is refused, and says which; the handle then iterates as its twin does
    twin2, dev2 = gp.ChainSolver(O.POSE2, landmark_dim=2), gp.ChainSolver(O.POSE2, landmark_dim=2)
    for s in (twin2, dev2):
        S.apply(p, s)
        s.set_landmarks(lm + 0.1)
        s.add_landmark_priors([0, 1], lm, np.full((2, 2), 0.5))
        s.add_range([1], [1], [np.linalg.norm(lm[1] - p["pose"][1, :2])], [0.1])
        s.add_range(at, which, z, np.full(6, 0.1))
        s.compile()
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*range factor 0.*landmark 1"):
        dev2.marginalize_head(k)
    assert dev2.N == N
    for a, b in zip(run3(twin2), run3(dev2)):
        assert np.array_equal(a, b)
    assert np.array_equal(twin2.get_landmarks(), dev2.get_landmarks())


# ---------------------------------------------------------------- 5. sliding equals batch
def test_sliding_window_equals_batch():
    p = S.linear_chain(64)
    orc = S.apply(p, O.Chain(p["kind"]))
    for _ in range(2):
        orc.iterate_gn()
    bp, bv = orc.get_states()
    window, step = 16, 4
    dev = solver(FL.sub_problem(p, 0, window))
    lo, hi = 0, window
    for _ in range(12):
        dev.marginalize_head(step)
        dev.append_states(p["pose"][hi:hi + step], p["vel"][hi:hi + step])
        new = FL.sub_problem(p, lo + step, hi + step, new_from=hi)
        dev.add_gp_priors(new["gp_left"], new["gp_dt"])
        dev.add_pose_priors(new["prior_idx"], new["prior_pose"], new["prior_sig"])
        lo, hi = lo + step, hi + step
        dev.compile()
        dev.iterate_gn()
        dev.iterate_gn()
    dp, dv = dev.get_states()
    assert dp.shape[0] == window and hi == 64
    assert np.abs(dp - bp[48:]).max() <= 1e-9 and np.abs(dv - bv[48:]).max() <= 1e-9


# ---------------------------------------------------------------- 6. twice equals once
def test_marginalising_twice_equals_once():
    tol = lam_tol()
    p = problem("pose2", 12, 5)
    a, b = solver(p), solver(p)
    a.marginalize_head(3)
    a.compile()
    a.marginalize_head(2)
    b.marginalize_head(5)
    _, _, La, ga = a.get_head_prior()
    _, _, Lb, gb = b.get_head_prior()
    _, _, sD, sg = head_reference(p, 5)
    eL, eg = float(np.abs(La - Lb).max()) / sD, float(np.abs(ga - gb).max()) / sg
    print("twice against once: %.3g (Lambda), %.3g (gamma) relative; tolerance %.3g" % (eL, eg, tol))
    assert eL <= tol and eg <= tol


# ---------------------------------------------------------------- 7. a head without absolute information
def test_gauge_free_head():
    N, k = 12, 4
    q = problem("linear3", N)
    p = {key: v for key, v in q.items() if not key.startswith(("prior_", "vprior", "between_"))}
    at = np.array([6, 9], dtype=np.int32)
    p.update(prior_idx=at, prior_pose=q["pose"][at] + 0.1, prior_sig=np.full((2, 3), 0.05))
    orc = S.apply(p, O.Chain(p["kind"]))
    dev = solver(p)
    dev.marginalize_head(k)          # no GPSLAM_E_NOT_SPD
    dev.compile()
    orc.iterate_gn()
    dev.iterate_gn()
    bp, bv = orc.get_states()
    dp, dv = dev.get_states()
    assert np.abs(dp - bp[k:]).max() <= 1e-9 and np.abs(dv - bv[k:]).max() <= 1e-9


# ---------------------------------------------------------------- 8. the contract
def refused(dev, code, *args):
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(%d\)" % code):
        dev.marginalize_head(*args)


def run3(dev):
    for _ in range(3):
        dev.iterate_gn()
    return dev.get_states()


def test_refusals_leave_the_handle_as_it_was():
    p = problem("pose2", 12, 5)
    twin, dev = solver(p), solver(p)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-1\)"):
        dev.get_head_prior()
    refused(dev, -1, 0)
    refused(dev, -1, 12)
    refused(dev, -1, -3)
    assert dev.N == 12
    for a, b in zip(run3(twin), run3(dev)):
        assert np.array_equal(a, b)
    # a loop closure that reaches into the head
    pc = S.add_loop_closures(problem("pose2", 12, 5), [(1, 9)])
    twin, dev = solver(pc), solver(pc)
    refused(dev, -5, 3)
    assert dev.N == 12
    for a, b in zip(run3(twin), run3(dev)):
        assert np.array_equal(a, b)
    dev.marginalize_head(1)          # ... and one that does not
    dev.compile()
    dev.iterate_gn()
    # not compiled: before compile(), and after a successful call
    raw = gp.ChainSolver(O.POSE2)
    raw.set_states(p["pose"], p["vel"])
    refused(raw, -4, 3)
    ok = solver(p)
    ok.marginalize_head(3)
    refused(ok, -4, 3)


def all_three_refused(h, q, why):
    """marginalize_head, add_state_gaussians and append_states answer GPSLAM_E_UNSUPPORTED and name the reason"""
    b = h.b
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*" + why):
        h.marginalize_head(3)
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*" + why):
        h.add_state_gaussians([0], q["pose"][:1], q["vel"][:1], np.eye(b)[None], np.zeros((1, b)))
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\).*" + why):
        h.append_states(q["pose"][:1], q["vel"][:1])
    assert h.N == q["pose"].shape[0]


@pytest.mark.parametrize("what", ["fp32", "sharded", "segmented"])
def test_unsupported_handles_refuse_and_iterate_as_their_twin(what):
    """compiled handles of a full problem: the refusals change nothing, the handle stays compiled and iterates bit-identically"""
    if what == "segmented":
        q = dict(S.pose2_range_chain(60, L=8, seed=1))
        q["prior_sig"] = np.full_like(q["prior_sig"], 1e-3)
        kw = dict(landmark_dim=2, force_segmented=True)
    else:
        q = problem("pose2", 12, 5)
        kw = dict(precision=gp.chain.FP32) if what == "fp32" else dict(force_sharded=True)
    twin, dev = solver(q, **kw), solver(q, **kw)
    all_three_refused(dev, q, what)
    for a, b in zip(run3(twin), run3(dev)):
        assert np.array_equal(a, b)
    # ... and before compile() the answer is the same, not GPSLAM_E_NOT_COMPILED
    raw = gp.ChainSolver(O.POSE2, **kw)
    raw.set_states(q["pose"], q["vel"])
    all_three_refused(raw, q, what)


def test_a_piece_of_a_split_chain_is_refused():
    """A piece iterates only through its driver's phases with the other pieces (iterate_gn refuses it), so there is no twin to
    iterate against: the three answers, and the states as they were set."""
    p = problem("pose2", 12, 5)
    h = gp.ChainSolver(O.POSE2)
    h.set_states(p["pose"], p["vel"])
    h.fs_set_split(0, 2)
    all_three_refused(h, p, "split")
    pose, vel = h.get_states()
    assert np.array_equal(pose, p["pose"]) and np.array_equal(vel, p["vel"])
    assert h.get_state_gaussians()[0].size == 0


def test_rot3_bias_is_refused():
    pb = S.rot3_bias_ahrs_chain(12)
    twin, hb = solver(pb), solver(pb)
    refused(hb, -5, 3)
    assert hb.N == 12
    for a, b in zip(run3(twin), run3(hb)):
        assert np.array_equal(a, b)
    hb.add_state_gaussians([0], pb["pose"][:1], pb["vel"][:1], np.eye(12)[None], np.zeros((1, 12)))
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-5\)"):
        hb.compile()


# ---------------------------------------------------------------- 9. the state Gaussian's rows through the fused level 0
@pytest.mark.parametrize("name", ["pose3", "linear3"])
def test_window_of_thousands_of_states_takes_the_fused_level0(name):
    """The cases above have one solver level.  4100 states (not a multiple of any chunk) after marginalize_head(100): the b rows of
    the prior go through k_fused_level0 -- the SE(3) record chain with odd rows, and block size 6 -- and the launch census says so.
    Two Gauss-Newton steps against a GPSLAM_PLAN_UNFUSED_LEVEL0 handle of the same graph (k_assemble_ghost + k_chunk_forward_rows) at
    1e-9 of the states' scale, the bound and the measure (test_gpu_parity.states_close) that tests/test_gpu_forms.py holds every
    fused form to against that handle."""
    p = S.pose3_chain(4100) if name == "pose3" else S.linear_chain(4100)
    out = []
    for plan in (0, gp.PLAN_UNFUSED_LEVEL0):
        dev = solver(p, plan=plan)
        dev.marginalize_head(100)
        dev.compile()
        dev.launch_census()
        dev.iterate_gn()
        census = dev.launch_census()
        dev.iterate_gn()
        out.append((census, dev.get_head_prior(), dev.get_states()))
        dev.close()
    (cf, hf, sf), (cu, hu, su) = out
    print("%s: fused handle l0_fused %d block %d sv %d odd_rows %d; unfused handle l0_fused %d l0_rows %d"
          % (name, cf["l0_fused"], cf["block"], cf["sv"], cf["odd_rows"], cu["l0_fused"], cu["l0_rows"]))
    assert cf["l0_fused"] == 1 and cf["block"] == (12 if name == "pose3" else 6) and cu["l0_fused"] == 0
    if name == "pose3":
        assert cf["odd_rows"] >= 1
    print("Lambda of the two handles differs by %.3g of its largest entry" % (np.abs(hf[2] - hu[2]).max() / np.abs(hu[2]).max()))
    assert np.abs(hf[2]).max() > 0.0
    states_close(p["kind"], su[0], su[1], sf[0], sf[1], 1e-9)


def test_reruns_are_bit_identical():
    p = problem("pose3", 12, 5)
    out = []
    for _ in range(2):
        dev = solver(p)
        dev.marginalize_head(5)
        dev.compile()
        dev.iterate_gn()
        out.append((dev.get_head_prior(), dev.get_states()))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        assert np.array_equal(a, b)
