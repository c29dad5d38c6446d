"""The algebra of loop closures in column passes (tests/closure_passes_model.py) against a direct dense solve: H0 from the oracle's
normal_equations() of a closure-free chain, U random blocks at random state pairs, slices of 1, 4 and 9 closures.  Runs without a GPU;
the device's Y is checked only through the step (tests/test_gpu_closure_passes.py)."""
import numpy as np
import pytest

from oracle import oracle as O
from gpslam_amd import synthetic as S
import closure_passes_model as M


def _strip_landmarks(p):
    return {k: v for k, v in p.items() if not (k.startswith("range_") or k.startswith("lprior") or k.startswith("landmark"))}


def _anchored(p):
    q = dict(p)
    q["prior_sig"] = np.full_like(p["prior_sig"], 1e-3)
    return q


def _refined_solve(H, b):
    """A dense solve with three steps of iterative refinement, residuals in long double: the reference, and the model's stand-in
    for a run of the chain solver.  H0 of these chains has condition 1e7; plain LAPACK solves of X and of the slices of Z, each
    rounded its own way, leave the model 1e-14 .. 1e-10 of |x| from the reference depending on the slicing (measured at 120
    states: SE(2), 12 closures, w = 1 / 4 / 9 / 12: 1e-14, 1.2e-14, 7.2e-11, 1.1e-12) -- rounding of the stand-in, not algebra.  What the device's
    own factorisation leaves is measured on the device (tests/test_gpu_closure_passes.py)."""
    x = np.linalg.solve(H, b)
    Hl = H.astype(np.longdouble)
    for _ in range(3):
        res = (b.astype(np.longdouble) - Hl @ x.astype(np.longdouble)).astype(np.float64)
        x = x + np.linalg.solve(H, res)
    return x


@pytest.fixture(scope="module")
def chains():
    out = {}
    p2 = _anchored(_strip_landmarks(S.pose2_range_chain(90, seed=9)))
    D, Ob, g, _, _, _ = S.apply(p2, O.Chain(O.POSE2)).normal_equations()
    out["pose2"] = (M.dense(D, Ob), g.reshape(-1), 6, 3)
    p3 = S.pose3_chain(45, seed=2)
    D, Ob, g, _, _, _ = S.apply(p3, O.Chain(O.POSE3)).normal_equations()
    out["pose3"] = (M.dense(D, Ob), g.reshape(-1), 12, 6)
    return out


@pytest.mark.parametrize("w", [1, 4, 9])
@pytest.mark.parametrize("name,K", [("pose2", 12), ("pose2", 40), ("pose3", 6), ("pose3", 20)])
def test_passes_equal_the_direct_solve(chains, name, K, w):
    H0, g, b, d = chains[name]
    n = H0.shape[0]
    rng = np.random.default_rng(1000 * K + w)
    U, r, pairs = M.random_closures(n // b, b, d, K, rng)
    assert all(abs(i - j) > 1 for i, j in pairs)
    X, P, solves = M.solve_in_passes(H0, g[:, None], U, r, d, w, solve=_refined_solve)
    assert P == -(-K // w) and solves == P + 1
    ref = _refined_solve(H0 + U.T @ U, g + U.T @ r)
    err = np.abs(X[:, 0] - ref).max() / np.abs(ref).max()
    print("%s K %d w %d: P %d, |x - ref| / |ref| %.2e" % (name, K, w, P, err))
    assert err <= 1e-11


@pytest.mark.parametrize("w", [1, 4, 9])
def test_landmark_columns_ride_along(w):
    """[g | B] with the 8 landmark columns of a chain with four range landmarks (the oracle's own B): every column of the result is
    (H0 + U^T U)^-1 of its own right-hand side, U^T r in column 0 alone -- what the landmark Schur complement is formed from"""
    p = _anchored(S.pose2_range_chain(90, L=4, seed=3))
    D, Ob, g, B, _, _ = S.apply(p, O.Chain(O.POSE2, landmark_dim=2)).normal_equations()
    H0, b, d = M.dense(D, Ob), 6, 3
    n = H0.shape[0]
    rng = np.random.default_rng(77 + w)
    U, r, _ = M.random_closures(n // b, b, d, 10, rng)
    G = np.hstack([g.reshape(-1, 1), B.reshape(n, -1)])
    assert G.shape[1] == 9
    X, P, solves = M.solve_in_passes(H0, G, U, r, d, w, solve=_refined_solve)
    assert P == -(-10 // w) and solves == P + 1
    G[:, 0] += U.T @ r
    ref = _refined_solve(H0 + U.T @ U, G)
    # The bound is 1e-11 of |x|inf of the solution [x | H^-1 B].  Per column, for the record: a landmark column of the result is the
    # difference of two larger ones (H0^-1 B and H0^-1 U^T Y, H0 being softer than H), so it carries their rounding -- measured
    # 3e-14 .. 6e-12 of the column's own largest entry on this chain for every slicing alike (up to 2.5e-11 at 120 states), 1e-15 of
    # the solution's.
    for c in range(G.shape[1]):
        print("w %d column %d: |x - ref| / |ref column| %.2e" % (w, c, np.abs(X[:, c] - ref[:, c]).max() / np.abs(ref[:, c]).max()))
    err = np.abs(X - ref).max() / np.abs(ref).max()
    print("w %d: |x - ref| / |ref| %.2e" % (w, err))
    assert err <= 1e-11
