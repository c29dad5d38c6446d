"""numpy model of loop closures in column passes (closures.hpp CloPass, api_impl.inc launch_solve_passes) on dense matrices.

H = H0 + U^T U with H0 everything but the closures and U (nc x n) their whitened rows.  One linear solve is
    X  = H0^-1 [g + 0 | B]                      pass 0, which also carries slice 0 of U^T as extra columns
    Z_s = H0^-1 U_s^T                           one pass per slice s of w closures; only W = U [X | Z] is kept of them
    Y  = (I + 1/2 (U Z + (U Z)^T))^-1 ([r | 0] - U X)
    X_full = X + H0^-1 (U^T Y)                  the final pass, U^T Y in place of [g | B]
and X_full = (H0 + U^T U)^-1 [g + U^T r | B]: column 0 the update, the others the landmark columns the Schur complement is formed
from.  Every `solve` below is one run of the chain solver on the device; the model only fixes what rides in which pass."""
import numpy as np


def dense(D, O):
    """block-tridiagonal H0 from diagonal blocks D and O[i] = A_{i+1,i} (normal_equations' convention)"""
    N, b = D.shape[0], D.shape[1]
    A = np.zeros((N * b, N * b))
    for i in range(N):
        A[i * b:(i + 1) * b, i * b:(i + 1) * b] = D[i]
        if i + 1 < N:
            A[(i + 1) * b:(i + 2) * b, i * b:(i + 1) * b] = O[i]
            A[i * b:(i + 1) * b, (i + 1) * b:(i + 2) * b] = O[i].T
    return A


def random_closures(N, b, d, K, rng):
    """K closures at random pairs |i - j| > 1 (any order, states may repeat): U (K d x N b) with a d x d block on the pose columns of
    either state, r (K d), and the pairs"""
    U = np.zeros((K * d, N * b))
    pairs = []
    for k in range(K):
        while True:
            i, j = (int(v) for v in rng.integers(0, N, 2))
            if abs(i - j) > 1:
                break
        pairs.append((i, j))
        U[k * d:(k + 1) * d, i * b:i * b + d] = rng.standard_normal((d, d)) * 30.0
        U[k * d:(k + 1) * d, j * b:j * b + d] = rng.standard_normal((d, d)) * 30.0
    return U, rng.standard_normal(K * d), pairs


def solve_in_passes(H0, G, U, r, d, w, solve=np.linalg.solve):
    """X_full (n x ncols) for right-hand sides G = [g | B] (n x ncols; U^T r is NOT in g) with slices of w closures.
    solve(H0, rhs) stands for one run of the chain solver.  Returns (X_full, passes P, solves of H0).

    The identity holds for ONE operator H0^-1.  The device applies the same factorisation to every column of every pass; LAPACK's
    solve rounds a column differently depending on how many ride with it, and with cond(H0) = 1e7 such inconsistencies between X
    and Z show at 1e-10 of |x| -- whoever wants the algebra alone to 1e-11 passes an accurate solve."""
    n, ncols = G.shape
    nc = U.shape[0]
    K = nc // d
    P = -(-K // w)
    W = np.zeros((nc, ncols + nc))
    X = None
    solves = 0
    for p in range(P):
        k0, k1 = p * w, min((p + 1) * w, K)
        Us = U[k0 * d:k1 * d]
        rhs = np.hstack([G, Us.T]) if p == 0 else np.hstack([np.zeros_like(G), Us.T])   # (later passes: the lead columns are not read)
        sol = solve(H0, rhs)
        solves += 1
        if p == 0:
            X = sol[:, :ncols].copy()
            W[:, :ncols] = U @ X                                   # the gather's ncols leading columns
        W[:, ncols + k0 * d:ncols + k1 * d] = U @ sol[:, ncols:]   # ... and the slice's own
    WZ = W[:, ncols:]
    S = np.eye(nc) + 0.5 * (WZ + WZ.T)
    R = -W[:, :ncols]
    R[:, 0] += r
    L = np.linalg.cholesky(S)
    Y = np.linalg.solve(L.T, np.linalg.solve(L, R))
    Xf = X + solve(H0, U.T @ Y)                           # the final pass and k_clo_add
    solves += 1
    return Xf, P, solves
