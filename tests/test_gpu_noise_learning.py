"""The measurement-noise statistic and the predicted covariances on the device (gpslam_hip_meas_noise_statistic,
gpslam_hip_meas_predicted_covariances; gpslam_amd/csrc/meas_noise.hip) against the numpy model, and evidence.learn_meas_noise.

Reference: inv of the oracle's dense H at the device's states, with the oracle's linearize_meas() there
(noise_learning_model.statistic).  Bound, entrywise, from the tolerances the project already holds (as DESIGN 4k's): the marginals
are held to tol_of(H) relative to dg dg^T (dg = sqrt(diag Sigma)), the host and factor arithmetic to 1e-11, so
    |B - B_ref| <= tol_of(H) sum_m |J| (dg dg^T) |J|^T + 1e-11 (sum_m |e| |e|^T + |B_ref|),
for Bw with R J and R e, for P per factor (without the error term).  The reference is computed a second way, Sigma from a Cholesky
factor of H instead of inv, and must itself sit inside the bound.

Seen on one MI355X (worst |device - reference| over the bound): the family's graphs at most 1.8e-3 (se3 projection, P), their robust
twins' P 6.8e-3 (se3 GPS), the 257 workgroups 5.7e-4 of the 1e-11 terms; learn_meas_noise at most 1.8e-13 from the model against
3.4e-10."""
import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import evidence as EV
from gpslam_amd import synthetic as S
from oracle import oracle as O
import fixed_lag_mix_model as FM
import marginals_mix_model as MX
import noise_learning_model as NM
from test_gpu_marginals import oracle_H, solver, gn, tol_of
from test_gpu_marginals_mix import device, here, robust_reference
from test_gpu_closure_passes import _info, _pairs
from test_gpu_closure import _anchored
from test_gpu_evidence import _census_counts

pytestmark = pytest.mark.gpu
REL = 1e-11
RUN = 32        # factors per workgroup of k_mn_stat (kMnRun)
ODO, GPS, RANGE, IRANGE = gp.chain.MEAS_ODOMETRY2D, gp.chain.MEAS_INTERP_GPS, gp.chain.MEAS_RANGE, gp.chain.MEAS_INTERP_RANGE


def reference(H, e, J, idx, lm, R, N, ld, two, use=None, tol=None):
    """((B, Bw, n, P, scales), (bound of B, of Bw, of P))"""
    tol = tol_of(H) if tol is None else tol
    ref = NM.statistic(np.linalg.inv(H), e, J, idx, lm, R, use, N=N, ld=ld, two=two)
    bounds = NM.bounds(tol, ref, ref[4], REL)
    Linv = np.linalg.inv(np.linalg.cholesky(H))
    two_ = NM.statistic(Linv.T @ Linv, e, J, idx, lm, R, use, N=N, ld=ld, two=two)
    for x, y, bd in zip((ref[0], ref[1], ref[3]), (two_[0], two_[1], two_[3]), bounds):
        assert np.all(np.abs(x - y) <= bd)
    return ref, bounds


def check(what, dev, kind, ref, bounds, use=None, P=True):
    B, Bw, n = dev.meas_noise_statistic(kind, use)
    got = [("B", B, ref[0], bounds[0]), ("Bw", Bw, ref[1], bounds[1])]
    if P:
        Pd = dev.meas_predicted_covariances(kind)
        assert np.array_equal(Pd, np.swapaxes(Pd, 1, 2))
        got.append(("P", Pd, ref[3], bounds[2]))
    assert n == ref[2], (n, ref[2])
    assert np.array_equal(B, B.T) and np.array_equal(Bw, Bw.T)
    for name, x, y, bd in got:
        worst = (np.abs(x - y) / np.maximum(bd, 1e-300)).max() if x.size else 0.0
        print("%s %s: n %d, |.| %.3g, worst |dev - ref| / bound %.3g (largest bound %.3g)" % (what, name, n, np.abs(y).max() if y.size else 0.0, worst, bd.max() if bd.size else 0.0))
        assert np.all(np.abs(x - y) <= bd), (what, name, worst)
    return B, Bw, n


def description_reference(ph, pre, H, use=None, tol=None):
    """the reference of one kind of a plain description at its own states"""
    mk, idx, lm, two, rows, ld, R = NM.kind_of(ph, pre)
    e, J = MX.oracle(ph).linearize_meas(mk, len(idx))
    return (mk,) + reference(H, e, J, idx, lm, R, ph["pose"].shape[0], ld, two, use, tol)


# ---------------------------------------------------------------- 1. the family's graphs
def _ds2(p):
    """se3 with Cal3DS2 on the second projection call (nine calibration numbers; zeros on the first call are Cal3_S2's)"""
    q = dict(p)
    dist = np.where((p["proj_call"] == 0)[:, None], 0.0, np.array([0.05, -0.02, 1e-3, -5e-4]))
    q["proj_K"] = np.hstack([p["proj_K"], dist])
    return q


@pytest.mark.parametrize("name", list(FM.NS) + ["se3_ds2"])
def test_every_kind_of_every_graph(name):
    """interpolated range, range, attitude, GPS with sigmas and with full covariances, odometry2d, bearing-range, projection (Cal3_S2,
    Cal3DS2), body_P_sensor, the VW family, SE(2) in the first-order chart; at the initial states and after two Gauss-Newton steps.
    Every kind arrives in two or three calls, each in a shuffled order of its states: no permutation is the identity"""
    p = _ds2(MX.graph("se3")) if name == "se3_ds2" else MX.graph(name)
    dev = device(p)
    done = 0
    for steps in MX.STEPS:
        gn(dev, steps - done)
        done = steps
        ph = here(p, dev)
        H = MX.H_of(ph)
        dev.marginals()
        assert NM.kinds(p)
        for pre in NM.kinds(p):
            mk, ref, bounds = description_reference(ph, pre, H)
            idx = np.asarray(p[FM.MEAS[pre][1]])
            assert np.any(np.diff(idx) < 0)
            check("%s %s after %d steps" % (name, pre, steps), dev, mk, ref, bounds)


@pytest.mark.parametrize("name", MX.ROBUST_GRAPHS)
def test_robust_twins(name):
    """predicted covariances on a robust graph: the unweighted J, Sigma of the reweighted H; the statistic refuses a used factor with a
    loss and accepts the others"""
    p = MX.graph(name, robust=True)
    dev = device(p)
    gn(dev, 2)
    ph, H, tol = robust_reference("robust " + name, p, dev)
    dev.marginals()
    for pre in FM.robust_kinds(p):
        loss = np.asarray(p[pre + "_loss"])
        use = loss == 0
        mk, ref, bounds = description_reference(FM.plain(ph), pre, H, use, tol)
        P = dev.meas_predicted_covariances(mk)
        worst = (np.abs(P - ref[3]) / np.maximum(bounds[2], 1e-300)).max()
        print("robust %s %s P: worst %.3g of the bound" % (name, pre, worst))
        assert np.all(np.abs(P - ref[3]) <= bounds[2])
        with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*robust loss"):
            dev.meas_noise_statistic(mk)
        if use.any():
            check("robust %s %s, the factors without a loss" % (name, pre), dev, mk, ref, bounds, use=use, P=False)


# ---------------------------------------------------------------- 2. shapes where the kernel can go wrong
def _odo_pair(N, left, seed=0, every=3):
    """a 2-D linear chain (LINEAR3: x, y, theta) with odometry factors on the intervals `left`, in that order; (p, dev, orc, sigmas)"""
    p = S.linear_chain(N, D=3, every=every)
    rng = np.random.default_rng(100 + seed)
    left = np.asarray(left, dtype=np.int32)
    M = len(left)
    d = p["pose"][left + 1] - p["pose"][left]
    c, s = np.cos(p["pose"][left, 2]), np.sin(p["pose"][left, 2])
    sig = 0.05 * (1.0 + rng.random((M, 3)))
    meas = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], d[:, 2]], axis=1) + sig * rng.standard_normal((M, 3))
    pair = []
    for sv in (gp.ChainSolver(gp.LINEAR3), O.Chain(O.LINEAR3)):
        S.apply(p, sv)
        sv.add_odometry2d(left, meas, sig)
        sv.compile()
        pair.append(sv)
    return p, pair[0], pair[1], sig


def _odo_reference(dev, orc, left, sig, use=None):
    H = oracle_H(orc, dev)
    e, J = orc.linearize_meas(ODO, len(left))
    R = np.stack([np.diag(1.0 / s) for s in sig])
    return reference(H, e, J, left, None, R, dev.N, 0, True, use)


@pytest.mark.parametrize("M", [1, RUN - 1, RUN, RUN + 1, 63, 64, 65])
def test_factor_counts_around_a_workgroups_run(M):
    """M factors on 24 states in a shuffled order: five to an interval, the next two intervals empty, the last interval among them --
    a run of 32 begins in the middle of an interval's five"""
    N = 24
    rng = np.random.default_rng(M)
    slots = np.concatenate([np.repeat(np.arange(0, N - 1, 3), 5), np.full(5, N - 2)])
    left = rng.permutation(np.sort(slots)[-M:] if M < len(slots) else np.concatenate([slots, rng.integers(0, N - 1, M - len(slots))]))
    assert (N - 2) in left and (M == 1 or np.any(np.diff(left) < 0))
    p, dev, orc, sig = _odo_pair(N, left, seed=M)
    gn(dev, 1)
    dev.marginals()
    ref, bounds = _odo_reference(dev, orc, left, sig)
    check("%d odometry factors" % M, dev, ODO, ref, bounds)


def test_use_masks():
    N, M = 24, 65
    rng = np.random.default_rng(5)
    left = rng.integers(0, N - 1, M)
    p, dev, orc, sig = _odo_pair(N, left, seed=1)
    gn(dev, 1)
    dev.marginals()
    one = np.zeros(M, bool)
    one[40] = True
    for what, use in (("all", np.ones(M, bool)), ("alternating", np.arange(M) % 2 == 0), ("one factor", one)):
        ref, bounds = _odo_reference(dev, orc, left, sig, use)
        check("use: " + what, dev, ODO, ref, bounds, use=use, P=False)
    dev.launch_census()
    before = _census_counts(dev)
    B, Bw, n = dev.meas_noise_statistic(ODO, np.zeros(M, bool))
    assert n == 0 and np.all(B == 0.0) and np.all(Bw == 0.0) and _census_counts(dev) == before
    with pytest.raises(gp.GpslamHipError, match="entries"):
        dev.meas_noise_statistic(ODO, np.ones(M + 1, bool))
    assert dev.meas_noise_statistic(RANGE)[2] == 0 and dev.meas_predicted_covariances(RANGE).shape == (0, 1, 1)


def test_gps_with_tau_outside_the_interval():
    """SE(3), 4 interpolated GPS factors per interval in a shuffled order, tau from -0.3 dt to 1.4 dt"""
    p = dict(S.pose3_gps_chain(10, per_interval=4, keep_odometry=True))
    M = len(p["gps_left"])
    rng = np.random.default_rng(2)
    order = rng.permutation(M)
    for k in ("gps_left", "gps_meas", "gps_sigma", "gps_dt", "gps_tau"):
        p[k] = p[k][order]
    p["gps_tau"] = p["gps_dt"] * rng.uniform(-0.3, 1.4, M)
    assert (p["gps_tau"] < 0).any() and (p["gps_tau"] > p["gps_dt"]).any()
    dev = solver(p)
    orc = S.apply(p, O.Chain(O.POSE3))
    gn(dev, 2)
    dev.marginals()
    H = oracle_H(orc, dev)
    e, J = orc.linearize_meas(GPS, M)
    R = np.stack([np.diag(1.0 / s) for s in p["gps_sigma"]])
    ref, bounds = reference(H, e, J, p["gps_left"], None, R, dev.N, 0, True)
    check("gps, tau outside", dev, GPS, ref, bounds)


# ---------------------------------------------------------------- 3. many partials without a dense inverse
def test_linear3_chain_of_257_workgroups():
    """257 * 32 odometry factors: k_mn_reduce adds 257 partials.  No dense inverse of 49350 x 49350: Sigma_m comes from the device's
    own S / S_next (pinned to the model by tests/test_gpu_marginals.py), so only the 1e-11 terms of the bound stay, with
    sum |J| |Sigma_m| |J|^T in the place of the covariance scale"""
    N = 257 * RUN + 1
    left = np.random.default_rng(3).permutation(N - 1)
    p, dev, orc, sig = _odo_pair(N, left, every=10)
    gn(dev, 1)
    dev.marginals()
    Sd, Sn = dev.get_marginals()
    orc.set_states(*dev.get_states())
    e, J = orc.linearize_meas(ODO, N - 1)
    R = np.stack([np.diag(1.0 / s) for s in sig])
    ref = NM.statistic((Sd, Sn, None, None), e, J, left, None, R, N=N, two=True)
    assert ref[2] == 257 * RUN
    sc = ref[4]
    bounds = (REL * (sc["cov"] + sc["err"] + np.abs(ref[0])), REL * (sc["cov_w"] + sc["err_w"] + np.abs(ref[1])), REL * (sc["cov_P"] + np.abs(ref[3])))
    check("linear3, 257 workgroups", dev, ODO, ref, bounds)


# ---------------------------------------------------------------- 4. landmarks and closures
def _plaza(closures=None):
    p = _anchored(S.pose2_range_chain(60, L=4, seed=3))
    N = p["N"]
    # plain ranges too, in a shuffled order, the last state among them
    rng = np.random.default_rng(11)
    idx = rng.permutation(np.concatenate([np.arange(0, N, 4), [N - 1]])).astype(np.int32)
    lm = rng.integers(0, 4, len(idx)).astype(np.int32)
    z = np.linalg.norm(p["landmark_truth"][lm] - p["truth"][idx, :2], axis=1) + 0.3 * rng.standard_normal(len(idx))
    p.update(prange_idx=idx, prange_lm=lm, prange_z=z, prange_sigma=0.3 * (1.0 + rng.random(len(idx))))
    if closures is not None:
        p = S.add_loop_closures(p, closures, seed=5)
    return p


def _plaza_pair(p, max_passes=None):
    dev = gp.ChainSolver(gp.POSE2, landmark_dim=2, chart=gp.CHART_FIRST_ORDER)
    if max_passes is not None:
        dev.set_closure_passes(max_passes, 0)
    orc = O.Chain(O.POSE2, chart=O.CHART_FIRST_ORDER, landmark_dim=2)
    for sv in (dev, orc):
        S.apply(p, sv)
        sv.add_range(p["prange_idx"], p["prange_lm"], p["prange_z"], p["prange_sigma"])
        sv.compile()
    return dev, orc


def _plaza_check(what, p, dev, orc):
    H = oracle_H(orc, dev, p if "closure_first" in p else None)
    for kind, key, two in ((IRANGE, "range", True), (RANGE, "prange", False)):
        idx, lm = p[key + ("_left" if two else "_idx")], p[key + "_lm"]
        e, J = orc.linearize_meas(kind, len(idx))
        R = (1.0 / np.asarray(p[key + "_sigma"])).reshape(-1, 1, 1)
        ref, bounds = reference(H, e, J, idx, lm, R, dev.N, 2, two)
        B, _, _ = check("%s, %s" % (what, key), dev, kind, ref, bounds)
        # a wrong landmark column fails: the reference with every factor's landmark moved on by one is outside the bound
        wrong = NM.statistic(np.linalg.inv(H), e, J, idx, (lm + 1) % 4, R, N=dev.N, ld=2, two=two)
        assert np.any(np.abs(B - wrong[0]) > bounds[0]) and np.any(np.abs(dev.meas_predicted_covariances(kind) - wrong[3]) > bounds[2])


def test_plaza_like_pose2_with_four_landmarks():
    """60 states, first-order chart: Sxl and Slm enter; a plain range on state N - 1 never reads state N"""
    p = _plaza()
    assert p["prange_idx"].max() == p["N"] - 1
    dev, orc = _plaza_pair(p)
    gn(dev, 2)
    dev.marginals()
    _plaza_check("plaza", p, dev, orc)


@pytest.mark.parametrize("K,max_passes,info", [(3, None, (3, 3, 1)), (8, 32, (8, 6, 2))])
def test_plaza_like_with_closures_in_one_pass_and_in_column_passes(K, max_passes, info):
    """4 landmarks leave room for 6 closures in a pass (1 + 8 + 3 w <= 28): 3 closures in one pass, 8 in two with the kept Z"""
    p = _plaza([[0, 59], [59, 3], [1, 30]] + _pairs(60, K - 3, 21) if K > 3 else [[0, 59], [59, 3], [1, 30]])
    dev, orc = _plaza_pair(p, max_passes)
    _info(dev, *info)
    if info[2] > 1:
        dev.marginals_keep_closure_columns()
    gn(dev, 2)
    dev.marginals()
    _plaza_check("plaza, %d closures" % K, p, dev, orc)


def test_segmented_handle():
    """the family's 2-D linear graph on the segmented landmark path: the kinds that name a landmark are refused, odometry is
    accepted with marginals_on_segments and agrees with the dense-border handle"""
    p = MX.graph("r3")
    dense = device(p)
    gn(dense, 2)
    seg = device(p, force_segmented=True, segment_length=8)
    assert seg.segment_plan()["active"] == 1
    seg.set_states(*dense.get_states())
    seg.set_landmarks(dense.get_landmarks())
    seg.marginals_on_segments()
    seg.marginals()
    for pre in ("prange", "brange"):
        for call in (seg.meas_noise_statistic, seg.meas_predicted_covariances):
            with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*segmented landmark path"):
                call(FM.MEAS[pre][0])
    ph = here(p, seg)
    mk, ref, bounds = description_reference(ph, "odo", MX.H_of(ph))
    B, _, _ = check("segmented r3, odometry", seg, mk, ref, bounds)
    dense.marginals()
    assert np.all(np.abs(dense.meas_noise_statistic(mk)[0] - B) <= 2 * bounds[0])


# ---------------------------------------------------------------- 5. the handle
def test_stale_and_refused_calls_carry_their_message_and_launch_nothing():
    left = np.arange(20)
    p, dev, orc, sig = _odo_pair(21, left)

    def refused(d, pattern, kind=ODO):
        for call in (d.meas_noise_statistic, d.meas_predicted_covariances):
            d.launch_census()
            before = _census_counts(d)
            with pytest.raises(gp.GpslamHipError, match=pattern):
                call(kind)
            assert _census_counts(d) == before, pattern

    refused(dev, r"\(-1\).*stale")                  # before marginals
    dev.marginals()
    dev.meas_noise_statistic(ODO)
    dev.set_meas_covariance(ODO, np.eye(3)[None] * 0.01)
    refused(dev, r"\(-1\).*stale")
    dev.compile()
    dev.marginals()
    dev.meas_noise_statistic(ODO)
    dev.iterate_gn()
    refused(dev, r"\(-1\).*stale")
    dev.marginals()
    dev.set_states(*dev.get_states())
    refused(dev, r"\(-1\).*stale")
    refused(solver(S.rot3_bias_ahrs_chain(40)), r"\(-5\).*ROT3_BIAS", gp.chain.MEAS_AHRS)
    refused(solver(S.linear_chain(30, D=3), precision=1), r"\(-5\).*fp32")
    refused(solver(S.linear_chain(30, D=3), force_sharded=True), r"\(-5\).*sharded")
    refused(dev, r"\(-5\).*MEAS_AHRS", gp.chain.MEAS_AHRS)
    assert gp.chain._noise_lib().gpslam_hip_meas_noise_statistic(dev._h, 8, None, None, None, None) == -1


def test_no_interference_and_determinism():
    p = MX.graph("se3")
    a, b = device(p), device(p)
    gn(a, 2)
    gn(b, 2)
    a.marginals()
    before = a.get_marginals(cross=True)
    first = [a.meas_noise_statistic(FM.MEAS[pre][0]) for pre in NM.kinds(p)]
    Pf = [a.meas_predicted_covariances(FM.MEAS[pre][0]) for pre in NM.kinds(p)]
    after = a.get_marginals(cross=True)             # (still valid: no "stale")
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    second = [a.meas_noise_statistic(FM.MEAS[pre][0]) for pre in NM.kinds(p)]
    for f, s_, P, pre in zip(first, second, Pf, NM.kinds(p)):
        assert np.array_equal(f[0], s_[0]) and np.array_equal(f[1], s_[1]) and f[2] == s_[2] == len(p[FM.MEAS[pre][1]])
        assert np.array_equal(f[0], f[0].T) and np.array_equal(f[1], f[1].T)
        assert np.array_equal(P, a.meas_predicted_covariances(FM.MEAS[pre][0]))
    for _ in range(3):
        ra, sa = a.iterate_gn()
        rb, sb = b.iterate_gn()
        assert (ra, sa.error_before, sa.error_after, sa.delta_inf_norm) == (rb, sb.error_before, sb.error_after, sb.delta_inf_norm)
    for x, y in zip(MX.states_of(a, p), MX.states_of(b, p)):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------- 6. learning
from noise_learning_model import C_TRUE, learn_problem, model_learn, tight as _tight  # noqa: E402


@pytest.mark.parametrize("mode,with_qc", [("scale", False), ("rows", False), ("shared", False), ("scale", True)])
def test_learn_meas_noise_follows_the_model_step_by_step(mode, with_qc):
    """from 3 x the truth (rows: the truth's diagonal): every theta / C of the device's sequence is held to the numpy model run on
    the oracle by the rule of DESIGN section 2 for soft graphs -- 1e-9 plus ten times the distance between the model and its own
    twin started 1e-15 away.  (That the MODEL's fixed point lies within 6 standard errors of the truth is a condition on the seed:
    tests/test_noise_learning_model.py checks it on the CPU.)"""
    p = learn_problem()
    M = len(p["gps_left"])
    start = 3.0 * (np.diag(np.diag(C_TRUE)) if mode == "rows" else C_TRUE)
    steps = 6
    qc = (np.asarray(p["qc"]), True) if with_qc else None
    ref = model_learn(p, mode, start, steps, _tight(O.default_params()), qc)
    twin = model_learn(p, mode, start * (1.0 + 1e-15), steps, _tight(O.default_params()), qc)
    dev = solver(p)
    out = EV.learn_meas_noise(dev, GPS, p["pose"], p["vel"], params=_tight(dev.default_params()), steps=steps, rtol=0.0, mode=mode,
                              with_qc=qc, cov0=start)
    assert len(out) == steps
    for k, (got, logz, iters) in enumerate(out):
        th, q = (got if with_qc else (got, None))
        scale = np.abs(ref[k][0]).max()
        tol = 1e-9 * scale + 10.0 * np.abs(ref[k][0] - twin[k][0]).max()
        gap = np.abs(np.asarray(th) - ref[k][0]).max()
        print("%s step %d: %s, |dev - model| %.3g of %.3g, log Z %s, %d iterations" % (mode, k, np.asarray(th).reshape(-1)[:3], gap, tol, logz, iters))
        assert gap <= tol
        if with_qc:
            tq = 1e-9 * np.abs(ref[k][1]).max() + 10.0 * np.abs(ref[k][1] - twin[k][1]).max()
            assert np.abs(q - ref[k][1]).max() <= tq
