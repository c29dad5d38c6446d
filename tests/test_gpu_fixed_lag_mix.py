"""Fixed-lag smoothing on the device with every factor and noise model in the head (gpslam_amd/csrc/fixedlag.hip: each_factor_array,
keep_of, k_head_left, k_head_left_lm, k_head_sums, k_border_inject, k_head_schur, k_head_schur_border) against the oracle's arrays and
the numpy models of tests/fixed_lag_model.py, tests/fixed_lag_border_model.py and tests/fixed_lag_mix_model.py.

Graphs (fixed_lag_mix_model.graph; 12 to 16 states, k = 1, 5, N - 1; with marginalize_head_onto_landmarks and without it, then without
the head's landmark factors):
  se2     SE(2), both charts: a Qc per interval on half the GP priors; interpolated ranges without a sensor offset and with two different
          ones; plain ranges; 3 landmarks with priors
  se3     SE(3): interpolated GPS with diagonal sigmas, with a sensor transform and with full covariances in one table; interpolated
          projection to 4 landmarks through two calibrations, one with a sensor transform; interpolated ranges without and with one
  se3_vw  SE(3) with world velocities: interpolated GPS without and with a sensor transform
  so3     SO(3): interpolated attitude, a Qc per interval on half the GP priors
  r3      the linear (x, y, theta) chain with planar landmarks: odometry2d, bearing-range and range to 3 landmarks
Every sigma, tau, dt, k, covariance and Qc differs from factor to factor, every kind arrives in two or three calls (without the option,
then with it), each call in a seeded shuffled order of its states, so that a survivor which inherits a deleted neighbour's entry moves
the result far beyond the bounds below.

(a) Lambda, gamma of the head against the model on the oracle's arrays: within lam_tol() = 100 x the largest distance, over the cases
of this file, between the model run in float64 and in np.longdouble, relative to max |diag| of the head's share (gamma: max |g|);
asserted to lie in (0, 1e-10).  The factor 100 is the one tests/test_gpu_fixed_lag.py gives for the device's other summation order.
Robust cases add how far the model itself moves when every weight moves by 1e-13 relative (the bound tests/test_gpu_robust.py holds
the device's weights to).
(b) One Gauss-Newton step after marginalize_head(k) and compile() against the oracle's batch step at 1e-9, the project's per-step
bound; two more against the model's step on the tail-only oracle chain that carries the device's prior.
Robust cases: the reference is the oracle on reweighted(p, w), w = np_loss of each factor's own (loss, k) at the whitened norm of a
plain device handle's linearize_meas errors; after the step of (b) meas_weights of the survivors, in their order, at 1e-13."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpslam_amd as gp
from oracle import oracle as O
from helpers import pose_close
import fixed_lag_model as FL
import fixed_lag_border_model as FB
import fixed_lag_mix_model as FM

pytestmark = pytest.mark.gpu

FAMILY = [(n, k, onto, 0) for n, k, onto in FM.family()] + [(n, k, onto, 1) for n, k, onto in FM.family() if n == "se2"]
# (se2 without the landmark option keeps no measurement factor in its head: every kind of it names a landmark)
ROBUST = [(n, k, onto) for n, k, onto in FM.family() if n in ("se3", "r3") or (n == "se2" and onto)]
INNER = [("se2", True), ("se3", False)]


def device(p, onto, **kw):
    dev = FM.apply(p, FM.chain(p, gp.ChainSolver, **kw))
    if onto:
        dev.marginalize_head_onto_landmarks()
    return dev


def oracle(p):
    return FM.apply(p, FM.chain(p))


# ---------------------------------------------------------------- the references, computed once
@functools.lru_cache(maxsize=None)
def plain_case(name, k, onto, chart):
    return FM.case(name, k, onto, chart=chart)


@functools.lru_cache(maxsize=None)
def long_case(name, N, k):
    return FM.case(name, k, name == "se2", N=N)


@functools.lru_cache(maxsize=None)
def long_reference(name, N, k, longdouble=False):
    return FM.head_reference(long_case(name, N, k), k, name == "se2", np.longdouble if longdouble else np.float64)


def inner_gaussians(p, k, onto, seed=3):
    """random full-rank Gaussians on states 2, k - 1 and k, linearised a few tenths away from the current state: state Gaussians
    (idx, pose_lin, vel_lin, A, c), with `onto` border Gaussians (idx, pose_lin, vel_lin, lm_lin, A, c)"""
    rng = np.random.default_rng(seed)
    kind, d = p["kind"], O.TANGENT_DIM[p["kind"]]
    n = 2 * d + (p["landmarks"].size if onto else 0)
    out = []
    for i in (2, k - 1, k):
        pl = O.retract(kind, p["pose"][i], 0.3 * rng.standard_normal(d), p["chart"])
        vl = p["vel"][i] + 0.3 * rng.standard_normal(d)
        A, c = 20.0 * rng.standard_normal((n, n)), 20.0 * rng.standard_normal(n)
        out.append((i, pl, vl) + ((p["landmarks"] + 0.3 * rng.standard_normal(p["landmarks"].shape),) if onto else ()) + (A, c))
    return out


@functools.lru_cache(maxsize=None)
def inner_case(name, onto):
    p = FM.graph(name, FM.NS[name], 5, landmarks=onto)
    return p, inner_gaussians(p, 5, onto)


def distance(a, b):
    return max(float(np.abs(a[0] - b[0]).max()) / a[2], float(np.abs(a[1] - b[1]).max()) / a[3])


@functools.lru_cache(maxsize=None)
def lam_tol():
    worst = 0.0
    for name, k, onto, chart in FAMILY:
        p = plain_case(name, k, onto, chart)
        worst = max(worst, distance(FM.head_reference(p, k, onto), FM.head_reference(p, k, onto, np.longdouble)))
    for name, k, onto in ROBUST:      # (the weights at the oracle's residuals: the device's differ by rounding)
        p = FM.case(name, k, onto, robust=True)
        q = FM.reweighted(p, {pre: w for pre, (r, w) in FM.robust_weights(p, FM.plain_errors(p, oracle(FM.plain(p)))).items()})
        worst = max(worst, distance(FM.head_reference(q, k, onto), FM.head_reference(q, k, onto, np.longdouble)))
    for name, onto in INNER:
        p, gs = inner_case(name, onto)
        worst = max(worst, distance(FM.head_reference(p, 5, onto, gaussians=gs[:2]), FM.head_reference(p, 5, onto, np.longdouble, gaussians=gs[:2])))
    for name, N, k in FM.LONG:
        worst = max(worst, distance(long_reference(name, N, k), long_reference(name, N, k, True)))
    tol = 100.0 * worst
    print("model float64 against longdouble: %.3g relative; tolerance %.3g" % (worst, tol))
    assert 0.0 < tol < 1e-10
    return tol


# ---------------------------------------------------------------- the two checks
def head_prior(dev, onto):
    return dev.get_head_prior_border()[1:] if onto else dev.get_head_prior()[2:]


def check_a(what, dev, p, k, onto, ref, extra=0.0):
    """(a): the device's Lambda, gamma of the last marginalize_head against ref = (Lambda, gamma, scale, gscale)"""
    tol = lam_tol() + extra
    Lam, gam = head_prior(dev, onto)
    pl, vl = dev.get_head_prior()[:2]
    assert np.array_equal(pl, p["pose"][k]) and np.array_equal(vl, p["vel"][k])
    eL, eg = float(np.abs(Lam - ref[0]).max()) / ref[2], float(np.abs(gam - ref[1]).max()) / ref[3]
    print("%s: device against model %.3g (Lambda), %.3g (gamma) relative; tolerance %.3g" % (what, eL, eg, tol))
    assert eL <= tol and eg <= tol


def check_states(kind, dev, rp, rv, rl, tol=1e-9):
    dp, dv = dev.get_states()
    assert dp.shape == rp.shape
    assert np.abs(dv - rv).max() <= tol
    for a, b in zip(dp, rp):
        assert pose_close(kind, a, b, tol)
    if rl is not None:
        assert np.abs(dev.get_landmarks() - rl).max() <= tol


def prior_of(dev, p):
    """the Gaussians the handle carries, as the model's step takes them: state Gaussians on a graph without landmarks, else border
    Gaussians (a state Gaussian padded with zero landmark columns)"""
    idx, pl, vl, A, c = dev.get_state_gaussians()
    if "landmarks" not in p:
        return [(int(idx[f]), pl[f], vl[f], A[f], c[f]) for f in range(len(idx))]
    b, nl = dev.b, dev.L * dev.ld
    lm = dev.get_landmarks()
    out = []
    for f in range(len(idx)):
        Ap, cp = np.zeros((b + nl, b + nl)), np.zeros(b + nl)
        Ap[:b, :b], cp[:b] = A[f], c[f]
        out.append((int(idx[f]), pl[f], vl[f], lm, Ap, cp))
    idx, pl, vl, ll, A, c = dev.get_border_gaussians()
    return out + [(int(idx[f]), pl[f], vl[f], ll[f].reshape(dev.L, dev.ld), A[f], c[f]) for f in range(len(idx))]


def model_step(ref, p, gaussians):
    """one Gauss-Newton step of the oracle chain `ref` plus Gaussians: (pose, vel, landmarks or None)"""
    if "landmarks" in p:
        return FB.step(ref, p["kind"], p["chart"], gaussians)[:3]
    return FL.gn_step(ref, p["kind"], p["chart"], gaussians) + (None,)


def reweighted_at(p, errors_from):
    """robust p -> the plain description the oracle takes at p's states: weights from errors_from(plain(p))'s linearize_meas"""
    if not FM.robust_kinds(p):
        return p
    rw = FM.robust_weights(p, FM.plain_errors(p, errors_from(FM.plain(p))))
    return FM.reweighted(p, {pre: w for pre, (r, w) in rw.items()})


def track(dev, p, k, steps=2):
    """more steps: the model on the tail-only oracle chain, carrying the device's prior, from the device's states; a robust tail is
    reweighted at the model's own states before every step"""
    _, tail = FM.head_tail(p, k)
    tail["pose"], tail["vel"] = dev.get_states()
    if "landmarks" in p:
        tail["landmarks"] = dev.get_landmarks()
    prior = prior_of(dev, p)
    for _ in range(steps):
        rp, rv, rl = model_step(oracle(reweighted_at(tail, oracle)), p, prior)
        tail["pose"], tail["vel"] = rp, rv
        if rl is not None:
            tail["landmarks"] = rl
        dev.iterate_gn()
        check_states(p["kind"], dev, rp, rv, rl)


def check_b(dev, p, k, batch, steps=2):
    """(b): dev has marginalised k states of p; batch = (pose, vel, landmarks or None) of the batch step of the whole graph"""
    with pytest.raises(gp.chain.GpslamHipError, match=r"\(-4\)"):
        dev.iterate_gn()
    dev.compile()
    dev.iterate_gn()
    check_states(p["kind"], dev, batch[0][k:], batch[1][k:], batch[2])
    if steps:
        track(dev, p, k, steps)


def batch_step(q, gaussians=()):
    """the oracle's batch Gauss-Newton step of the plain description q (with Gaussians: the model's step on the oracle's arrays)"""
    orc = oracle(q)
    if gaussians:
        return model_step(orc, q, gaussians)
    orc.iterate_gn()
    return orc.get_states() + (orc.get_landmarks() if "landmarks" in q else None,)


# ---------------------------------------------------------------- 1. every graph, plain
@pytest.mark.parametrize("name,k,onto,chart", FAMILY)
def test_lambda_gamma(name, k, onto, chart):
    p = plain_case(name, k, onto, chart)
    dev = device(p, onto)
    dev.marginalize_head(k)
    assert dev.N == FM.NS[name] - k
    check_a("%s k = %d onto %d chart %d" % (name, k, onto, chart), dev, p, k, onto, FM.head_reference(p, k, onto))
    if "landmarks" in p:
        assert (dev.get_border_gaussians()[0].size, dev.get_state_gaussians()[0].size) == ((1, 0) if onto else (0, 1))


@pytest.mark.parametrize("name,k,onto,chart", FAMILY)
def test_one_step_equals_batch_then_tracks_the_model(name, k, onto, chart):
    p = plain_case(name, k, onto, chart)
    dev = device(p, onto)
    dev.marginalize_head(k)
    check_b(dev, p, k, batch_step(p))


# ---------------------------------------------------------------- 2. robust factors in the head
@functools.lru_cache(maxsize=None)
def robust_case(name, k, onto):
    """(the robust description, a plain device handle's errors, prefix -> (r, w) at them, the reweighted description)"""
    p = FM.case(name, k, onto, robust=True)
    h = device(FM.plain(p), False)
    errors = FM.plain_errors(p, h)
    h.close()
    rw = FM.robust_weights(p, errors)
    return p, errors, rw, FM.reweighted(p, {pre: w for pre, (r, w) in rw.items()})


def weights_of(dev, mk, count):
    buf = np.zeros(count + 1)
    n = dev._chk(dev.lib.gpslam_hip_get_meas_weights(dev._h, int(mk), C.c_void_p(buf.ctypes.data)), "get_meas_weights")
    assert n == count, (mk, n, count)
    return buf[:count]


@pytest.mark.parametrize("name,k,onto", ROBUST)
def test_robust_lambda_gamma(name, k, onto):
    p, errors, rw, q = robust_case(name, k, onto)
    FM.check_populations(p, rw, k)
    ref = FM.head_reference(q, k, onto)
    # how far the reference moves when the weights move by what the device's may differ by
    margin = 0.0
    for s in (1.0 + 1e-13, 1.0 - 1e-13):
        qs = FM.reweighted(p, {pre: w for pre, (r, w) in FM.robust_weights(p, errors, s).items()})
        margin = max(margin, distance(ref, FM.head_reference(qs, k, onto)))
    unweighted = distance(ref, FM.head_reference(FM.plain(p), k, onto))
    print("%s k = %d onto %d: the model moves by %.3g when the weights move by 1e-13, by %.3g without the weights" % (name, k, onto, margin, unweighted))
    assert unweighted > 1e-3      # a head linearised without its weights is this far from the reference
    dev = device(p, onto)
    dev.marginalize_head(k)
    check_a("robust %s k = %d onto %d" % (name, k, onto), dev, p, k, onto, ref, margin)


@pytest.mark.parametrize("name,k,onto", ROBUST)
def test_robust_step_weights_and_tracking(name, k, onto):
    p, _, rw, q = robust_case(name, k, onto)
    dev = device(p, onto)
    for pre, (r, w) in rw.items():      # before anything is deleted: every factor's weight
        assert np.abs(weights_of(dev, FM.MEAS[pre][0], len(w)) - w).max(initial=0.0) <= 1e-13
    dev.marginalize_head(k)
    check_b(dev, p, k, batch_step(q), steps=0)
    # the survivors' weights at the new states, in their surviving order
    _, tail = FM.head_tail(p, k)
    tail["pose"], tail["vel"] = dev.get_states()
    tail["landmarks"] = dev.get_landmarks()
    h = device(FM.plain(tail), False)
    rw_tail = FM.robust_weights(tail, FM.plain_errors(tail, h))
    h.close()
    for pre, (r, w) in rw_tail.items():
        got = weights_of(dev, FM.MEAS[pre][0], len(w))
        print("robust %s k = %d onto %d: %s weights of %d survivors differ by %.3g" % (name, k, onto, pre, len(w), np.abs(got - w).max() if len(w) else 0.0))
        assert len(w) == 0 or np.abs(got - w).max() <= 1e-13
    track(dev, p, k)


def test_reruns_are_bit_identical():
    p = robust_case("se3", 5, True)[0]
    out = []
    for _ in range(2):
        dev = device(p, True)
        dev.marginalize_head(5)
        dev.compile()
        dev.iterate_gn()
        weights = tuple(weights_of(dev, FM.MEAS[pre][0], int((np.asarray(p[FM.MEAS[pre][1]]) >= 5).sum())) for pre in FM.robust_kinds(p))
        out.append(dev.get_head_prior_border() + dev.get_states() + (dev.get_landmarks(),) + weights)
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 3. Gaussians inside the head
@pytest.mark.parametrize("name,onto", INNER)
def test_gaussians_inside_the_head(name, onto):
    k = 5
    p, gs = inner_case(name, onto)
    cols = list(zip(*gs))
    dev = device(p, onto)
    if onto:
        dev.add_border_gaussians(cols[0], cols[1], cols[2], np.stack(cols[3]), np.stack(cols[4]), np.stack(cols[5]))
    else:
        dev.add_state_gaussians(cols[0], cols[1], cols[2], np.stack(cols[3]), np.stack(cols[4]))
    dev.compile()
    dev.marginalize_head(k)
    check_a("%s with Gaussians on states 2 and %d" % (name, k - 1), dev, p, k, onto, FM.head_reference(p, k, onto, gaussians=gs[:2]))
    # the Gaussian on state k reaches the tail as it was, at index 0, beside the new prior
    got = dev.get_border_gaussians() if onto else dev.get_state_gaussians()
    assert list(got[0]) == [0, 0]
    want = gs[2][1:3] + ((gs[2][3].reshape(-1),) if onto else ()) + gs[2][-2:]
    for a, e in zip(got[1:], want):
        assert np.array_equal(a[0], e)
    check_b(dev, p, k, batch_step(p, gs))


# ---------------------------------------------------------------- 4. long heads
@pytest.mark.parametrize("name,N,k", FM.LONG)
def test_long_head(name, N, k):
    onto = name == "se2"
    p = long_case(name, N, k)
    dev = device(p, onto)
    info = dev.plan_info()
    print("%s N = %d: %s" % (name, N, info))
    assert info["levels"] > 1
    dev.marginalize_head(k)
    assert dev.N == N - k
    check_a("long %s N = %d k = %d" % (name, N, k), dev, p, k, onto, long_reference(name, N, k))
    check_b(dev, p, k, batch_step(p), steps=0)


# ---------------------------------------------------------------- 5. a sliding window with losses and sensor offsets
def test_sliding_window_with_losses_tracks_the_model():
    """16 states, a window of 8 slid by 2 four times: marginalize_head, append_states, the new factors of every kind,
    set_meas_robust on the new factors only; then one device step against the model's step on the window's tail description,
    reweighted with numpy weights at the current states, plus the device's prior.  rob, aidx and sqi shrink and grow."""
    N, W, step = 16, 8, 2
    p = FM.graph("se2", N, 8, robust=True, chart=1)
    dev = device(FM.window(p, 0, W), True)
    dev.iterate_gn()
    lo, hi, lossy = 0, W, 0
    for _ in range(4):
        dev.marginalize_head(step)
        dev.append_states(p["pose"][hi:hi + step], p["vel"][hi:hi + step])
        new = FM.window(p, lo + step, hi + step, new_from=hi)
        assert all(len(new[FM.MEAS[pre][1]]) for pre in ("range", "prange"))
        lossy += int((np.asarray(new["range_loss"]) != 0).sum())
        FM.add_factors(new, dev)
        lo, hi = lo + step, hi + step
        dev.compile()
        tail = FM.window(p, lo, hi)
        tail["pose"], tail["vel"] = dev.get_states()
        tail["landmarks"] = dev.get_landmarks()
        prior = prior_of(dev, p)
        assert len(prior) == 1 and prior[0][0] == 0
        rp, rv, rl = model_step(oracle(reweighted_at(tail, oracle)), p, prior)
        dev.iterate_gn()
        check_states(p["kind"], dev, rp, rv, rl)
        for pre in FM.robust_kinds(p):
            assert len(weights_of(dev, FM.MEAS[pre][0], len(tail[FM.MEAS[pre][1]]))) == len(tail[FM.MEAS[pre][1]])
    assert hi == N and dev.N == W and lossy > 0
