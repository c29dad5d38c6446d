"""The references of tests/test_gpu_marginals_mix.py on their own (tests/marginals_mix_model.py): CPU only.

Every graph the GPU tests compare on stays under tol_of's cap of 1e-7 (kappa_s of the Jacobi-scaled dense H is printed), at the
states the oracle itself reaches by the same number of Gauss-Newton steps (a robust graph reweighted at every step's states);
check_populations holds there; marginalising a head into a Gaussian leaves the covariance of what remains unchanged (1e-11 in
correlation units, the bound of tests/test_marginals_model.py's dense algebra); reweighted() with unit weights is the plain H to the bit."""
import numpy as np
import pytest

from gpslam_amd import chain as GC
from oracle import oracle as O
import fixed_lag_mix_model as FM
import marginals_mix_model as MX
from test_gpu_marginals import tol_of

EPS = np.finfo(float).eps


def kappa(H):
    s = np.sqrt(np.diag(H))
    return float(np.linalg.cond(H / np.outer(s, s)))


def under_the_cap(what, H):
    k = kappa(H)
    tol = tol_of(H)      # (asserts its cap)
    print("%s: kappa_s %.3g, tol_of %.3g" % (what, k, tol))
    assert np.isfinite(k) and 100 * EPS * k <= 1e-7
    return tol


@pytest.mark.parametrize("steps", MX.STEPS)
@pytest.mark.parametrize("name", list(FM.NS))
def test_plain_graphs_stay_under_the_cap(name, steps):
    p = MX.gn(MX.graph(name), steps)
    under_the_cap("%s after %d steps" % (name, steps), MX.H_of(p))


@pytest.mark.parametrize("steps", MX.STEPS)
@pytest.mark.parametrize("name", MX.ROBUST_GRAPHS)
def test_robust_graphs_populations_and_cap(name, steps):
    p = MX.gn(MX.graph(name, robust=True), steps)
    q, rw = MX.reweighted_at(p)
    FM.check_populations(p, rw, 5)
    dead = sum(int((w == 0.0).sum()) for r, w in rw.values())
    print("%s after %d steps: %d factors at w = 0" % (name, steps, dead))
    assert dead >= 1
    H = MX.H_of(q)
    under_the_cap("robust %s after %d steps" % (name, steps), H)
    # the probe of the weight allowance moves the reference, and leaving the weights out moves it by orders of magnitude more
    Sig = np.linalg.inv(H)
    N, b = p["pose"].shape[0], 2 * O.TANGENT_DIM[p["kind"]]
    near = MX.moved(Sig, np.linalg.inv(MX.H_of(MX.reweighted_at(p, scale=1.0 + 1e-11)[0])), N, b)
    far = MX.moved(Sig, np.linalg.inv(MX.H_of(FM.plain(p))), N, b)
    print("the reference moves by %.3g when the weights move by 1e-11, by %.3g without the weights" % (near, far))
    assert near < 1e-9 and far > 1e-3


@pytest.mark.parametrize("steps", MX.STEPS)
def test_the_other_three_losses(steps):
    p = MX.gn(MX.swap_losses(MX.graph("se2", robust=True)), steps)
    q, rw = MX.reweighted_at(p)
    FM.check_populations(p, rw, 5, losses=tuple(MX.OTHER.values()))
    under_the_cap("se2 with Geman-McClure, Welsh and Fair after %d steps" % steps, MX.H_of(q))


@pytest.mark.parametrize("name", ["se2", "se3", "r3"])
def test_unit_weights_are_the_plain_H_to_the_bit(name):
    p = MX.graph(name, robust=True)
    ones = {pre: np.ones(len(p[FM.MEAS[pre][1]])) for pre in FM.robust_kinds(p)}
    assert np.array_equal(MX.H_of(FM.reweighted(p, ones)), MX.H_of(FM.plain(p)))


# ---------------------------------------------------------------- marginalising the head leaves the rest's covariance alone
@pytest.mark.parametrize("name,k,onto,robust", MX.SCHUR)
def test_schur_identity_on_the_oracles_arrays(name, k, onto, robust):
    p = MX.schur_case(name, k, onto, robust)
    if robust:
        FM.check_populations(p, MX.weights_at(p), k)
    q, _ = MX.reweighted_at(p)
    H = MX.H_of(q)
    under_the_cap("%s k = %d onto %d" % (name, k, onto), H)
    Sig = np.linalg.inv(H)
    _, tail = FM.head_tail(q, k)
    Ht = MX.H_of(tail, lambdas=[(0, MX.head_lambda(q, k, onto))])
    N, b = q["pose"].shape[0], 2 * O.TANGENT_DIM[q["kind"]]
    e = MX.worst(Sig, MX.blocks(np.linalg.inv(Ht), N - k, b), first=k)
    print("%s k = %d onto %d: the tail with the head's Lambda against the whole graph %.3g" % (name, k, onto, e))
    assert e <= 1e-11


@pytest.mark.parametrize("name,onto", [("se2", True), ("se3_vw", False)])
def test_slid_window_stays_under_the_cap(name, onto):
    """the window of the GPU test after its slide, at the initial states (the GPU test takes one step there)"""
    p = MX.graph(name)
    N, k = FM.NS[name], 5
    Lam = MX.head_lambda(FM.window(p, 0, N - 2), k, onto)
    H = MX.H_of(FM.window(p, k, N), lambdas=[(0, Lam)])
    under_the_cap("%s slid by %d" % (name, k), H)
    far = MX.moved(np.linalg.inv(H), np.linalg.inv(MX.H_of(FM.window(p, k, N))), N - k, 2 * O.TANGENT_DIM[p["kind"]])
    print("without the head's Lambda the reference moves by %.3g" % far)
    assert far > 1e-3


def test_direct_gaussians_stay_under_the_cap():
    p = MX.graph("so3")
    H = MX.H_of(p, gaussians=MX.direct_gaussians(p))
    under_the_cap("so3 with two state Gaussians", H)
    for drop in (0, 1):      # a handle that lost A^T A of either Gaussian is this far from the reference
        Hd = MX.H_of(p, gaussians=MX.direct_gaussians(p)[1 - drop:2 - drop])
        far = MX.moved(np.linalg.inv(H), np.linalg.inv(Hd), FM.NS["so3"], 6)
        print("without A^T A of Gaussian %d the reference moves by %.3g" % (drop, far))
        assert far > 1e-3


# ---------------------------------------------------------------- loop closures and the segmented case
@pytest.mark.parametrize("name", ["pose2_5", "pose2_5_lm", "pose2_12", "pose3_6"])
def test_robust_closure_graphs(name):
    p, chart, _ = MX.closure_graph(name)
    pose, vel, lm = MX.closure_gn(p, chart, MX.CLOSURE_STEPS)
    r, w = MX.closure_weights(p, pose, chart)
    print("%s: r %s\nw %s" % (name, np.round(r, 3), np.round(w, 4)))
    MX.check_closure_populations(p, r, w)
    H = MX.closure_H(MX.closure_reweighted(p, w), chart, pose, vel, lm)
    under_the_cap(name, H)
    # an unweighted J_c (every w = 1) is this far from the reference
    Hu = MX.closure_H(MX.closure_reweighted(p, np.ones(len(w))), chart, pose, vel, lm)
    far = MX.moved(np.linalg.inv(H), np.linalg.inv(Hu), len(pose), 2 * O.TANGENT_DIM[p["kind"]])
    print("with unweighted closures the reference moves by %.3g" % far)
    assert far > 1e-3


def test_segmented_graph():
    p = MX.gn(MX.segmented_graph(), MX.SEGMENTED_STEPS)
    q, rw = MX.reweighted_at(p)
    r, w = rw["range"]
    huber = np.arange(len(r)) % 2 == 0
    FM.check_populations(p, rw, 5, losses=(GC.ROBUST_HUBER, GC.ROBUST_CAUCHY))
    assert (w[huber] < 1).sum() >= 3 and (w[huber] == 1).sum() >= 3
    under_the_cap("segmented, %d ranges, %d Huber weights below 1" % (len(r), int((w[huber] < 1).sum())), MX.H_of(q))
