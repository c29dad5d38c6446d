"""The numpy model of fixed-lag smoothing with landmarks (tests/fixed_lag_border_model.py) against dense algebra on the oracle's
arrays: CPU only.

The border recursion against a dense Schur complement of the assembled head at 1e-11 (relative to max |diag| of the head's share of
[D_k ; H_LL], and to max |g|, |g_L|); Lambda's eigenvalues at or above -1e-10 of the largest; the factorisation of a rank-deficient
Lambda; and the Gauss-Newton step of the tail plus the prior against the batch step of the whole graph at 1e-11 -- the prior is the
exact marginal of the head's linearisation, and both steps linearise at the same point."""
import numpy as np
import pytest

from helpers import pose_close
from oracle import oracle as O
import fixed_lag_border_model as FB

CASES = [("pose2", 3), ("pose2", 13), ("pose3", 9), ("linear3", 3)]
KS = [1, 2, 5, 11]


@pytest.mark.parametrize("name,L", CASES)
@pytest.mark.parametrize("k", KS)
def test_border_recursion_against_dense_schur(name, L, k):
    p = FB.border_problem(name, 12, k, L)
    arrays = FB.head_arrays(p, k)
    Lam, gam, scale, gscale = FB.schur_border(*arrays, k)
    Lam_d, gam_d = FB.schur_border_dense(*arrays, k)
    eL, eg = np.abs(Lam - Lam_d).max() / scale, np.abs(gam - gam_d).max() / gscale
    L1, g1, _, _ = FB.schur_border(*arrays, k, np.longdouble)
    print("%s L = %d k = %d: recursion against dense %.3g / %.3g; float64 against longdouble %.3g / %.3g"
          % (name, L, k, eL, eg, np.abs(Lam - L1).max() / scale, np.abs(gam - g1).max() / gscale))
    assert eL <= 1e-11 and eg <= 1e-11
    w = np.linalg.eigvalsh(0.5 * (Lam + Lam.T))
    assert w.min() >= -1e-10 * w.max()
    # landmark 0 is seen from the head, so its block of Lambda is not zero
    b = arrays[0].shape[1]
    assert np.abs(Lam[b:b + 2, b:b + 2]).max() > 0.0


@pytest.mark.parametrize("name,L,k", [("pose2", 13, 1), ("pose2", 3, 5), ("pose3", 9, 2)])
def test_factorisation_of_a_rank_deficient_lambda(name, L, k):
    p = FB.border_problem(name, 12, k, L)
    Lam, gam, scale, gscale = FB.schur_border(*FB.head_arrays(p, k), k)
    A, c = FB.factor(Lam, gam, scale)
    n = Lam.shape[0]
    rank = int((np.abs(A).max(axis=1) > 0).sum())
    print("%s L = %d k = %d: rank %d of %d" % (name, L, k, rank, n))
    if L == 13:
        assert rank < n          # landmarks the head never saw: zero rows of A
    assert np.abs(A.T @ A - 0.5 * (Lam + Lam.T)).max() <= 1e-11 * scale
    assert np.abs(A.T @ c + gam).max() <= 1e-11 * gscale


def batch_and_tail_steps(p, k, lam=0.0):
    kind = p["kind"]
    batch = FB.apply(p, FB.chain(p))
    bp, bv, bl, _ = FB.step(batch, kind, O.CHART_EXPMAP, [], lam)
    Lam, gam, scale, _ = FB.schur_border(*FB.head_arrays(p, k), k)
    A, c = FB.factor(Lam, gam, scale)
    _, tail = FB.head_tail(p, k)
    orc = FB.apply(tail, FB.chain(tail))
    prior = [(0, p["pose"][k], p["vel"][k], p["landmarks"], A, c)]
    tp, tv, tl, _ = FB.step(orc, kind, O.CHART_EXPMAP, prior, lam)
    return (bp[k:], bv[k:], bl), (tp, tv, tl)


@pytest.mark.parametrize("name,L", CASES)
@pytest.mark.parametrize("k", KS)
def test_tail_plus_prior_step_equals_batch_step(name, L, k):
    p = FB.border_problem(name, 12, k, L)
    (bp, bv, bl), (tp, tv, tl) = batch_and_tail_steps(p, k)
    assert np.abs(bv - tv).max() <= 1e-11 and np.abs(bl - tl).max() <= 1e-11
    for a, b in zip(bp, tp):
        assert pose_close(p["kind"], a, b, 1e-11)


def test_dense_step_is_the_oracles_step():
    """the dense reference step is the oracle's own Gauss-Newton iteration where the oracle can express the graph"""
    p = FB.border_problem("pose2", 12, 5, 3)
    a, b = FB.apply(p, FB.chain(p)), FB.apply(p, FB.chain(p))
    a.iterate_gn()
    pose, vel, lm, err = FB.step(b, p["kind"], O.CHART_EXPMAP, [])
    ap, av = a.get_states()
    assert np.abs(ap - pose).max() <= 1e-11 and np.abs(av - vel).max() <= 1e-11 and np.abs(a.get_landmarks() - lm).max() <= 1e-11
    assert abs(a.error() - err) <= 1e-11 * err


def test_gauge_free_head_factorises():
    p = FB.border_problem("pose2", 12, 4, 3, priors=False)
    Lam, gam, scale, gscale = FB.schur_border(*FB.head_arrays(p, 4), 4)
    A, c = FB.factor(Lam, gam, scale)
    assert int((np.abs(A).max(axis=1) > 0).sum()) < Lam.shape[0]
    assert np.abs(A.T @ A - 0.5 * (Lam + Lam.T)).max() <= 1e-11 * scale
