"""Powell's dogleg on the device (include/gpslam_hip_dogleg.h, gpslam_amd/csrc/dogleg.hip) against the numpy
model of tests/dogleg_model.py on the oracle's arrays.

Graphs (dogleg_model.FAMILY, SIZES): the families of tests/fixed_lag_mix_model.py at 12 to 16 states, with and without landmarks; two
states (one interval); 300 states on se3 and on se2 with landmarks (ten workgroups of k_dl_quad, a multi-block reduction); 1025 on se3
(33 workgroups, one state in the last); a GPSLAM_ROT3_BIAS chain of the AHRS recipe; a graph with a state Gaussian; one robust graph.

Bounds.  gg, gn, nn: 1e-11 relative, the bound the Jacobian rows are held to.  gHg is a sum whose terms can cancel: the larger of 1e-11
and ten times the distance between the model's block-form sum in float64 and in np.longdouble (the twin rule of DESIGN.md section 2;
tests/test_dogleg_model.py caps that distance at 1e-8 on every graph).  A kept step: 1e-9 relative, the project's per-step bound.  The
robust graph adds ten times what the model's own numbers move by when every acting weight is scaled by 1 + 1e-11, the bound the
device's weights are held to (tests/test_gpu_marginals_mix.py's rule).

Lockstep: trials, accepted and branch of every decidable iteration equal the model's exactly.  The trust radius equals the model's
exactly while it comes from the start by halving; once an iteration has set it to 3 |delta_d| it is a number computed from scalars that
are themselves held to 1e-11, and is held to 1e-10 relative.  What CAN be exact is (check_host_loop): every single-trial iteration is
replayed from the device's own numbers -- dogleg_last()'s scalars, the two costs of the stats -- through gpslam_hip_dogleg_point and
gpslam_hip_dogleg_decide (coefficients, prediction, branch, keep, stay and the radius after: to the bit) and through the model's point
and decide (branch, keep, stay to the bit; the radius to the bit where it is halved, kept or 3 |delta_n|, and at 1e-14 where it is
3 |delta_d| of a scaled or blended step, the bound |delta_d| = Delta itself is held to between two float64 evaluations).

The branch-2 step is bit-identical in states (and landmarks) to iterate_gn on a twin built with GPSLAM_PLAN_UNFUSED_LEVEL0: same
launches, and k_dl_blend's 0 * g + 1 * dn is dn."""
import numpy as np
import pytest

import gpslam_amd as gp
from oracle import oracle as O
import fixed_lag_mix_model as FM
import marginals_mix_model as MX
import dogleg_model as DM
from test_dogleg_model import DECIDABLE, lockstep_run

pytestmark = pytest.mark.gpu
ROW_TOL = 1e-11
STEP_TOL = 1e-9
ALL = DM.FAMILY + DM.SIZES
IDS = ["%s%s%s" % (n, "_lm" if lm else "", "" if N is None else "_%d" % N) for n, lm, N in ALL]


def device(p, hook=None, **kw):
    """the description on a handle; hook(solver, p): further factors, added once the states and landmarks are set"""
    if hook is None:
        return FM.apply(p, FM.chain(p, gp.ChainSolver, **kw))
    s = FM.chain(p, gp.ChainSolver, **kw)
    s.set_qc(p["qc"])
    s.set_states(p["pose"], p["vel"])
    if "landmarks" in p:
        s.set_landmarks(p["landmarks"])
        s.add_landmark_priors(p["lprior_idx"], p["lprior"], p["lprior_sig"])
    hook(s, p)
    FM.add_factors(p, s)
    s.compile()
    return s


def ahrs_pair(N=24):
    """the GPSLAM_ROT3_BIAS chain of the AHRS recipe on the oracle and on the device"""
    from gpslam_amd import synthetic as S
    p = S.rot3_bias_ahrs_chain(N)
    return S.apply(p, O.Chain(p["kind"])), S.apply(p, gp.ChainSolver(p["kind"]))


@pytest.fixture(scope="module")
def reference():
    """per graph: the description and the model's numbers at its initial states (computed once, never written to)"""
    cache = {}

    def get(name, lm, N):
        key = (name, lm, N)
        if key not in cache:
            p = DM.graph(name, lm, N)
            H, gv, arr = DM.system(p)
            s4, dn = DM.scalars(H, gv, arr)
            cache[key] = dict(p=p, gv=gv, dn=dn, s4=[float(v) for v in s4], twin=DM.twin_distance(arr))
        return cache[key]
    return get


def check_scalars(what, got, want, twin, extra=0.0):
    names = ("gg", "gHg", "gn", "nn")
    tol = [ROW_TOL + extra, max(ROW_TOL, 10.0 * twin) + extra, ROW_TOL + extra, ROW_TOL + extra]
    err = [abs(g - w) / abs(w) for g, w in zip(got, want)]
    print("%s: %s" % (what, ", ".join("%s %.3g of %.3g" % (n, e, t) for n, e, t in zip(names, err, tol))))
    for n, e, t in zip(names, err, tol):
        assert e <= t, (what, n, e, t)


def states_close(dev, q, tol=STEP_TOL):
    """the device's states and landmarks against the description q's, relative to the largest entry of each array"""
    pose, vel = dev.get_states()
    worst = max(np.abs(pose - q["pose"]).max() / max(1.0, np.abs(q["pose"]).max()), np.abs(vel - q["vel"]).max() / max(1.0, np.abs(q["vel"]).max()))
    if "landmarks" in q:
        worst = max(worst, np.abs(dev.get_landmarks() - q["landmarks"]).max() / max(1.0, np.abs(q["landmarks"]).max()))
    assert worst <= tol, worst
    return worst


def check_host_loop(dev, st, delta_in, delta_out, mode):
    """a single-trial iteration replayed from the device's own numbers (module docstring)"""
    if st.trials != 1:
        return False
    last = dev.dogleg_last()
    a, b, norm, pred, branch = gp.dogleg_point(last[:4], delta_in)
    assert (a, b, pred, branch) == (last[4], last[5], last[6], int(last[7]))
    keep, stay, d, _ = gp.dogleg_decide((st.error_before, st.last_trial_error, pred, norm), mode, delta_in, 0)
    assert (d, stay) == (delta_out, False)
    assert bool(st.accepted) == (keep and not st.last_trial_error > st.error_before)
    ma, mb, mnorm, mpred, mbranch = DM.point(last[:4], delta_in)
    mkeep, mstay, md, _ = DM.decide(st.error_before, st.last_trial_error, mpred, mnorm, mode, delta_in, 0)
    assert (mbranch, mkeep, mstay) == (branch, keep, stay)
    if branch == 2 or md in (delta_in, delta_in / 2):
        assert md == delta_out
    else:
        assert abs(md - delta_out) <= 1e-14 * delta_out
    return True


# ---------------------------------------------------------------- 1. the four scalars
@pytest.mark.parametrize("name,lm,N", ALL, ids=IDS)
def test_scalars(reference, name, lm, N):
    ref = reference(name, lm, N)
    dev = device(ref["p"])
    dev.iterate_dogleg(1.0)
    check_scalars("%s N %s" % (name, N), dev.dogleg_last()[:4], ref["s4"], ref["twin"])


def test_scalars_on_the_ahrs_chain():
    orc, dev = ahrs_pair()
    arr = orc.normal_equations()
    s4, _ = DM.scalars(None, arr[2].reshape(-1), arr)
    dev.iterate_dogleg(1.0)
    check_scalars("rot3_bias", dev.dogleg_last()[:4], [float(v) for v in s4], DM.twin_distance(arr))


def test_scalars_with_a_state_gaussian():
    p = DM.graph("se2", True)
    rng = np.random.default_rng(5)
    b = 6
    A = np.triu(rng.standard_normal((b, b))) + 3.0 * np.eye(b)
    c = 0.1 * rng.standard_normal(b)
    lin_pose = O.retract(p["kind"], p["pose"][3], 0.05 * rng.standard_normal(3), p["chart"])
    lin_vel = p["vel"][3] + 0.05 * rng.standard_normal(3)
    H, gv, arr = DM.system(p, gaussians=[(3, lin_pose, lin_vel, A, c)])
    s4, _ = DM.scalars(H, gv, arr)
    dev = device(p, lambda s, q: s.add_state_gaussians([3], lin_pose, lin_vel, A, c))
    dev.iterate_dogleg(1.0)
    check_scalars("se2 + state Gaussian", dev.dogleg_last()[:4], [float(v) for v in s4], DM.twin_distance(arr))


# ---------------------------------------------------------------- 2. every branch
@pytest.mark.parametrize("name,lm,N", ALL, ids=IDS)
def test_every_branch(reference, name, lm, N):
    ref = reference(name, lm, N)
    p, (gg, gHg, gn, nn) = ref["p"], ref["s4"]
    nu, nnorm = np.sqrt((gg / gHg) ** 2 * gg), np.sqrt(nn)
    cases = [(0.5 * nu, 0), (2.0 * nnorm, 2)] + ([(0.5 * (nu + nnorm), 1)] if nu < nnorm else [])
    for delta, branch in cases:
        m = DM.iterate(p, delta, DM.ONE_STEP)
        assert (m["trials"], m["branch"], m["accepted"]) == (1, branch, True)      # (the model says what the case is)
        dev = device(p)
        st, d_after = dev.iterate_dogleg(delta, DM.ONE_STEP)
        last = dev.dogleg_last()
        assert (st.trials, st.accepted, int(last[7])) == (1, 1, branch)
        assert abs(d_after - m["delta"]) <= 1e-10 * m["delta"]
        assert check_host_loop(dev, st, delta, d_after, DM.ONE_STEP)
        worst = states_close(dev, m["p"])
        assert abs(st.error_after - m["error_after"]) <= STEP_TOL * m["error_after"]
        print("%s N %s branch %d: kept step %.3g of %.3g, error %.9g -> %.9g" % (name, N, branch, worst, STEP_TOL, st.error_before, st.error_after))
        if branch == 2:     # the Gauss-Newton step, to the bit
            twin = device(p, plan=gp.PLAN_UNFUSED_LEVEL0)
            twin.iterate_gn()
            for x, y in zip(dev.get_states(), twin.get_states()):
                assert np.array_equal(x, y)
            if lm:
                assert np.array_equal(dev.get_landmarks(), twin.get_landmarks())


# ---------------------------------------------------------------- 3. lockstep with the model
@pytest.mark.parametrize("start", DM.LOCKSTEP, ids=lambda s: s[0])
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_lockstep(start, mode):
    name, lm, scale, seed, delta = start
    run = lockstep_run(start, mode)
    dev = device(DM.perturbed(DM.graph(name, lm), scale, seed))
    halved = True       # the radius is still the start's, halved some number of times
    replayed = 0
    for it in range(DECIDABLE[(name, lm)][mode]):
        m = run[it]
        delta_in = delta
        st, delta = dev.iterate_dogleg(delta, mode)
        replayed += check_host_loop(dev, st, delta_in, delta, mode)
        got = (st.trials, st.accepted, int(dev.dogleg_last()[7]))
        print("%s mode %d iteration %d: trials, accepted, branch %s (model %s), delta %.17g (model %.17g)"
              % (name, mode, it, got, (m["trials"], int(m["accepted"]), m["branch"]), delta, m["delta"]))
        assert got == (m["trials"], int(m["accepted"]), m["branch"])
        halved = halved and np.log2(start[4] / m["delta"]) == np.round(np.log2(start[4] / m["delta"]))
        if halved:
            assert delta == m["delta"]
        else:
            assert abs(delta - m["delta"]) <= 1e-10 * m["delta"]
        assert abs(st.error_after - m["error_after"]) <= 1e-8 * m["error_after"]
    assert any(r["rejected"] for r in run[:DECIDABLE[(name, lm)][mode]])
    assert replayed >= 1      # (the searching mode takes several trials in most iterations of these starts)


# ---------------------------------------------------------------- 4. optimize_dogleg
@pytest.mark.parametrize("name,lm,N", DM.FAMILY, ids=IDS[:len(DM.FAMILY)])
def test_optimize(name, lm, N):
    p = DM.graph(name, lm, N)
    tol = dict(relative_error_tol=1e-12, absolute_error_tol=1e-12, max_iterations=50)
    q, iters, err, delta = DM.optimize(p, 1.0, DM.ONE_STEP, **tol)
    dev = device(p)
    rc, st = dev.optimize_dogleg(dev.default_params(**tol), 1.0, DM.ONE_STEP)
    print("%s: %d iterations (model %d), error %.12g (model %.12g)" % (name, st.iterations, iters, st.error_after, err))
    assert st.iterations == iters
    states_close(dev, q)
    # The fixed point, both optimisers driven until the cost stops falling.  A stop at a relative decrease of 1e-12 in the cost leaves
    # the states 1e-8 away from it along the weak directions of H (seen: 1.3e-8 on se3, 2.6e-8 on r3): the cost is flat there.
    floor = dict(relative_error_tol=0.0, absolute_error_tol=0.0, max_iterations=100)
    dog = device(p)
    rc, sd = dog.optimize_dogleg(dog.default_params(**floor), 1.0, DM.ONE_STEP)
    lmq = device(p)
    rc, sl = lmq.optimize(lmq.default_params(use_lm=1, **floor))
    pose, vel = lmq.get_states()
    worst = states_close(dog, MX.at(p, pose, vel, lmq.get_landmarks() if lm else None), 1e-8)
    print("%s: dogleg %d iterations to the floor, Levenberg-Marquardt %d; states differ by %.3g" % (name, sd.iterations, sl.iterations, worst))


# ---------------------------------------------------------------- 5. robust losses
def test_robust():
    p = DM.graph(DM.ROBUST, True, robust=True)
    H, gv, arr = DM.system(p)
    s4, _ = DM.scalars(H, gv, arr)
    # how far the model's own numbers move with the weights
    q, _ = MX.reweighted_at(p, scale=1.0 + 1e-11)
    arr2 = MX.oracle(q).normal_equations()
    gv2 = np.concatenate([arr2[2].reshape(-1), arr2[5]])
    s4b, _ = DM.scalars(MX.dense_H(arr2[0], arr2[1], arr2[3], arr2[4]), gv2, arr2)
    move = max(abs(float(a) - float(b)) / abs(float(a)) for a, b in zip(s4, s4b))
    # the allowance is capped: the scalars are at most quadratic in the weights (g linear, H linear, dn through H^-1), so a graph whose
    # numbers move by more than ten times the scaling of its weights is not a test graph
    print("robust %s: the model's scalars move by %.3g when the weights move by 1e-11: allowance %.3g (cap 1e-9)" % (DM.ROBUST, move, 10.0 * move))
    assert move <= 1e-10
    dev = device(p)
    f = DM.cost(p)
    assert abs(dev.error() - f) <= 1e-12 * f
    delta, prev = 1.0, None
    for it in range(6):
        st, delta = dev.iterate_dogleg(delta)
        if it == 0:
            assert abs(st.error_before - f) <= 1e-12 * f
            check_scalars("robust %s (the model moves by %.3g with the weights)" % (DM.ROBUST, move), dev.dogleg_last()[:4], [float(v) for v in s4],
                          DM.twin_distance(arr), 10.0 * move)
        assert st.error_after <= st.error_before
        assert prev is None or (st.error_after <= prev and abs(st.error_before - prev) <= 1e-12 * prev)      # (two kernels' sums of one cost)
        prev = st.error_after
        print("robust iteration %d: %.9g -> %.9g, %d trials, branch %d" % (it, st.error_before, st.error_after, st.trials, int(dev.dogleg_last()[7])))


# ---------------------------------------------------------------- 6. one solve per iteration
L0 = ("l0_fused", "l0_rows", "l0_column", "l0_column_fast", "top_chunk")


def test_one_solve_per_iteration():
    name, lm, scale, seed, delta = DM.THREE_TRIALS
    p = DM.perturbed(DM.graph(name, lm), scale, seed)
    dev, twin = device(p), device(p, plan=gp.PLAN_UNFUSED_LEVEL0)
    dev.launch_census()
    st, _ = dev.iterate_dogleg(delta, DM.SEARCH_EACH)
    a = dev.launch_census()
    twin.launch_census()
    twin.iterate_gn()
    b = twin.launch_census()
    print("trials %d; level-0 forward launches %s, Gauss-Newton twin %s" % (st.trials, {k: a[k] for k in L0}, {k: b[k] for k in L0}))
    assert st.trials >= 3
    assert sum(a[k] for k in L0) == sum(b[k] for k in L0) > 0
    assert a["retract"] == st.trials
    # ... and on the SE(3) chain that is planned for the fused level 0
    p3 = DM.graph("se3", False, 300)
    dev, twin = device(p3), device(p3, plan=gp.PLAN_UNFUSED_LEVEL0)
    dev.launch_census()
    st, _ = dev.iterate_dogleg(1e-3, DM.SEARCH_EACH)
    a = dev.launch_census()
    twin.launch_census()
    twin.iterate_gn()
    b = twin.launch_census()
    assert st.trials >= 3 and a["retract"] == st.trials and a["l0_fused"] == 0
    assert sum(a[k] for k in L0) == sum(b[k] for k in L0) > 0


# ---------------------------------------------------------------- 7. contract
def _closure(s, p):
    i, j = 1, p["pose"].shape[0] - 2
    s.add_between_pairs([i], [j], p["pose"][j:j + 1], np.full((1, O.TANGENT_DIM[p["kind"]]), 0.5))


def _border(s, p):
    n = s.b + p["landmarks"].size
    s.add_border_gaussians([0], p["pose"][0], p["vel"][0], p["landmarks"].reshape(-1), np.eye(n), np.zeros(n))


REFUSALS = [
    ("fp32", dict(precision=gp.FP32), None, "fp32", False),
    ("sharded", dict(force_sharded=True), None, "sharded", False),
    ("segmented", dict(force_segmented=True), None, "segmented", True),
    ("split", dict(force_segmented=True), lambda s, p: s.fs_set_split(0, 2), "split", True),
    ("closures", {}, _closure, "closures", True),
    ("border", {}, _border, "border Gaussians", True),
]


@pytest.mark.parametrize("what,kw,extra,message,lm", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_handle_as_it_was(what, kw, extra, message, lm):
    p = DM.graph("se2", lm, 60 if what in ("segmented", "split") else None)      # (segments need a chain to cut)

    def make():
        return device(p, extra, **kw)
    a, b = make(), make()
    before = a.get_states() + ((a.get_landmarks(),) if lm else ())
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*" + message):
        a.iterate_dogleg(1.0)
    with pytest.raises(gp.GpslamHipError, match=r"\(-5\).*" + message):
        a.optimize_dogleg()
    for x, y in zip(before, a.get_states() + ((a.get_landmarks(),) if lm else ())):
        assert np.array_equal(x, y)
    if what != "split":     # (a piece iterates only through its driver's phases with the other pieces: there its states as they were)
        a.iterate_gn()
        b.iterate_gn()
        for x, y in zip(a.get_states(), b.get_states()):
            assert np.array_equal(x, y)


def test_argument_errors():
    p = DM.graph("se2", True)
    dev = device(p)
    before = dev.get_states()
    for delta, mode in ((0.0, 0), (-1.0, 0), (float("inf"), 0), (float("nan"), 0), (1.0, 3), (1.0, -1)):
        with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
            dev.iterate_dogleg(delta, mode)
    with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
        dev.optimize_dogleg(delta_initial=0.0)
    for x, y in zip(before, dev.get_states()):
        assert np.array_equal(x, y)
    raw = FM.chain(p, gp.ChainSolver)
    raw.set_qc(p["qc"])
    raw.set_states(p["pose"], p["vel"])
    with pytest.raises(gp.GpslamHipError, match=r"\(-4\)"):
        raw.iterate_dogleg(1.0)


def test_a_non_positive_pivot_leaves_the_states_untouched():
    from gpslam_amd import synthetic as S
    p = S.linear_chain(20, D=3)
    q = dict(p)
    for k in ("prior_idx", "prior_pose", "prior_sig", "vprior_idx", "vprior", "vprior_sig"):
        q.pop(k)
    from test_gpu_marginals import solver
    dev = solver(q)
    before = dev.get_states()
    with pytest.raises(gp.GpslamHipError, match=r"\(-3\)"):
        dev.iterate_dogleg(1.0)
    for x, y in zip(before, dev.get_states()):
        assert np.array_equal(x, y)


def test_marginals_are_stale_after_an_iteration():
    dev = device(DM.graph("se2", True))
    dev.marginals()
    dev.get_marginals()
    dev.iterate_dogleg(1.0)
    with pytest.raises(gp.GpslamHipError, match="stale"):
        dev.get_marginals()


def test_reruns_are_bit_identical():
    name, lm, scale, seed, delta0 = DM.THREE_TRIALS
    p = DM.perturbed(DM.graph(name, lm), scale, seed)
    out = []
    for _ in range(2):
        dev, delta, rec = device(p), delta0, []
        for it in range(3):
            st, delta = dev.iterate_dogleg(delta, DM.SEARCH_EACH)
            rec.append((st.error_before, st.error_after, st.delta_inf_norm, st.trials, st.accepted, delta) + dev.dogleg_last())
        out.append((rec, dev.get_states(), dev.get_landmarks()))
    assert out[0][0] == out[1][0]
    for x, y in zip(out[0][1], out[1][1]):
        assert np.array_equal(x, y)
    assert np.array_equal(out[0][2], out[1][2])
    big = DM.graph("se3", False, 1025)
    last = []
    for _ in range(2):
        dev = device(big)
        dev.iterate_dogleg(1.0)
        last.append(dev.dogleg_last())
    assert last[0] == last[1]


def test_rot3_bias_pads_stay_zero():
    orc, dev = ahrs_pair()
    delta, branches = 0.05, []
    for it in range(3):
        st, delta = dev.iterate_dogleg(delta)
        assert st.error_after <= st.error_before
        branches.append(int(dev.dogleg_last()[7]))
    pose, vel = dev.get_states()
    print("rot3_bias: branches %s" % branches)
    assert np.abs(vel[:, 3:]).max() == 0.0
    assert set(branches) != {2}      # (a blend or a scaled gradient step went through k_dl_blend's pad rule)


def test_a_step_that_is_not_kept_restores_the_states():
    """A huge perturbation and a radius of 2e-5, as the model sees it: whatever the model's verdict, the device's is the same, and an
    iteration that keeps nothing leaves the states bit-identical.  (Host side, the floor itself: tests/test_dogleg_host.py.)"""
    p = DM.perturbed(DM.graph("se2", True), 1e3, 4)
    for mode in (0, 1, 2):
        m = DM.iterate(p, 2e-5, mode)
        dev = device(p)
        before = dev.get_states() + (dev.get_landmarks(),)
        st, delta = dev.iterate_dogleg(2e-5, mode)
        print("mode %d: accepted %d (model %d), trials %d, error %.6g -> %.6g, delta %.3g" % (mode, st.accepted, m["accepted"], st.trials, st.error_before, st.error_after, delta))
        assert st.accepted == int(m["accepted"]) and st.trials == m["trials"]
        if not st.accepted:
            assert st.error_after == st.error_before and st.delta_inf_norm == 0.0
            for x, y in zip(before, dev.get_states() + (dev.get_landmarks(),)):
                assert np.array_equal(x, y)


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_an_iteration_rejected_to_the_floor_keeps_nothing(mode):
    """Every trial's cost is not finite: a linear chain (H does not depend on the states, every pivot stays positive) set 1e200 away.
    The cost overflows to inf (which passes the NaN check of the linearisation point), g . g overflows, the blend coefficient is NaN,
    the trial states and f_new are NaN, rho is NaN: Delta 2e-5 -> 1e-5, once more, and at the floor the loop ends with nothing kept.
    The linearisation point is restored to the bit, and the handle iterates on as a twin that never made the call."""
    from gpslam_amd import synthetic as S
    from test_gpu_marginals import solver
    p = S.linear_chain(20, D=3)
    p = dict(p, pose=p["pose"] + 1e200, vel=p["vel"] - 1e200)
    dev, twin = solver(p), solver(p)
    before = dev.get_states()
    assert np.isinf(dev.error())
    st, delta = dev.iterate_dogleg(2e-5, mode)
    print("mode %d: accepted %d, trials %d, error %g -> %g (last trial %g), delta %g, last %s" % (mode, st.accepted, st.trials, st.error_before, st.error_after,
                                                                                         st.last_trial_error, delta, dev.dogleg_last()))
    assert (st.accepted, st.trials, delta) == (0, 2, 1e-5)
    assert st.error_after == st.error_before and st.delta_inf_norm == 0.0
    assert not np.isfinite(st.last_trial_error)
    for x, y in zip(before, dev.get_states()):
        assert np.array_equal(x, y)
    rc = [s_.lib.gpslam_hip_iterate_gn(s_._h, None) for s_ in (dev, twin)]
    assert rc[0] == rc[1]
    for x, y in zip(dev.get_states(), twin.get_states()):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.isfinite(dev.get_states()[0]).all()      # (the Gauss-Newton step of a linear problem lands at finite states)
