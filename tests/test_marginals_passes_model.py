"""The algebra of the marginals with closures in column passes (tests/marginals_passes_model.py) against the inverse of the dense H:
A from the oracle's normal_equations() of a closure-free chain, U random blocks at random state pairs, slices of 1, 4 and 9
closures, block sizes 6 and 12.  Bound: 1e-11 in correlation units, the bar of tests/closure_passes_model.py; as there, the dense
solves (the stand-in for the chain solver, and the reference inverse) are refined with long-double residuals, so that what is
measured is the algebra and not LAPACK's rounding at cond(A) = 1e7.  Runs without a GPU and passes on any code: it pins the formula
the device kernels implement (tests/test_gpu_marginals_passes.py holds those to the oracle)."""
import numpy as np
import pytest

from oracle import oracle as O
from gpslam_amd import synthetic as S
import closure_passes_model as CM
import marginals_passes_model as M
from test_closure_passes_model import _anchored, _refined_solve, _strip_landmarks


@pytest.fixture(scope="module")
def chains():
    out = {}
    p2 = _anchored(_strip_landmarks(S.pose2_range_chain(60, seed=9)))
    D, Ob, _, _, _, _ = S.apply(p2, O.Chain(O.POSE2)).normal_equations()
    out["pose2"] = (CM.dense(D, Ob), 6, 3)
    p3 = S.pose3_chain(40, seed=2)
    D, Ob, _, _, _, _ = S.apply(p3, O.Chain(O.POSE3)).normal_equations()
    out["pose3"] = (CM.dense(D, Ob), 12, 6)
    return out


def _corr_err(S_hat, S_ref, rows, cols):
    return float(np.max(np.abs(S_hat - S_ref) / np.outer(rows, cols)))


@pytest.mark.parametrize("w", [1, 4, 9])
@pytest.mark.parametrize("name,K", [("pose2", 12), ("pose2", 40), ("pose3", 6), ("pose3", 20)])
def test_sigma_xx_equals_the_dense_inverse(chains, name, K, w):
    A, b, d = chains[name]
    n = A.shape[0]
    rng = np.random.default_rng(2000 * K + w)
    U, _, pairs = CM.random_closures(n // b, b, d, K, rng)
    assert all(abs(i - j) > 1 for i, j in pairs)
    Sxx, Sll, Sxl, P = M.marginals_in_passes(A, U, d, w, solve=_refined_solve)
    assert P == -(-K // w) and Sll is None and Sxl is None
    ref = _refined_solve(A + U.T @ U, np.eye(n))
    dg = np.sqrt(np.diag(ref))
    err = _corr_err(Sxx, ref, dg, dg)
    print("%s K %d w %d: P %d, Sigma_xx against inv(H) in correlation units %.2e" % (name, K, w, P, err))
    assert err <= 1e-11


@pytest.mark.parametrize("w", [1, 4, 6])
def test_landmarks_and_closures_all_three_blocks(w):
    """the 8 landmark columns of a chain with four range landmarks (the oracle's own B and H_LL) beside 10 closures"""
    p = _anchored(S.pose2_range_chain(60, L=4, seed=3))
    D, Ob, _, B, HLL, _ = S.apply(p, O.Chain(O.POSE2, landmark_dim=2)).normal_equations()
    A, b, d = CM.dense(D, Ob), 6, 3
    n = A.shape[0]
    Bf = B.reshape(n, -1)
    assert Bf.shape[1] == 8
    rng = np.random.default_rng(99 + w)
    U, _, _ = CM.random_closures(n // b, b, d, 10, rng)
    Sxx, Sll, Sxl, P = M.marginals_in_passes(A, U, d, w, B=Bf, HLL=HLL, solve=_refined_solve)
    assert P == -(-10 // w)
    H = np.block([[A + U.T @ U, Bf], [Bf.T, HLL]])
    ref = _refined_solve(H, np.eye(n + 8))
    dg = np.sqrt(np.diag(ref))
    errs = (_corr_err(Sxx, ref[:n, :n], dg[:n], dg[:n]), _corr_err(Sll, ref[n:, n:], dg[n:], dg[n:]),
            _corr_err(Sxl, ref[:n, n:], dg[:n], dg[n:]))
    print("w %d: P %d, Sigma_xx / Sigma_LL / Sigma_xL against inv(H) in correlation units %.2e %.2e %.2e" % ((w, P) + errs))
    assert max(errs) <= 1e-11
