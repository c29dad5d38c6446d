"""numpy model of the marginals on a handle whose loop closures go in column passes (marginals.hip: k_mg_clo_inverse,
k_mg_clo_finish; api_impl.inc launch_solve_passes with keep_z) on dense matrices.

H = [[A + U^T U, B], [B^T, H_LL]] with A the chain part, U (nc x n) the closures' whitened rows, B the landmark coupling.  With
    Z_s = A^-1 U_s^T                            one pass per slice s of w closures, kept at EVERY state (the device's mg_Z)
    X   = A^-1 B                                pass 0's landmark columns
    M   = I + 1/2 (U Z + (U Z)^T)
    W   = X - A^-1 U^T M^-1 U X                 the final pass: (A + U^T U)^-1 B, the closure-corrected landmark columns
    S   = H_LL - B^T W
the blocks of Sigma = H^-1 are
    Sigma_xx = A^-1 + W S^-1 W^T - Z M^-1 Z^T,   Sigma_LL = S^-1,   Sigma_xL = -W S^-1.
Every `solve` stands for one run of the chain solver; the model fixes what is kept of which pass and how the terms combine."""
import numpy as np


def _ld(a):
    """The three terms of Sigma_xx are summed in long double: with stiff closures A^-1 is orders of magnitude larger than Sigma, and
    the model is about the algebra -- what fp64 sums leave of it is the device tests' subject, at their condition-number bound."""
    return np.asarray(a, dtype=np.longdouble)


def marginals_in_passes(A, U, d, w, B=None, HLL=None, solve=np.linalg.solve):
    """(Sigma_xx, Sigma_LL, Sigma_xL, passes P) with slices of w closures; Sigma_LL / Sigma_xL are None without landmarks"""
    n = A.shape[0]
    nc = U.shape[0]
    K = nc // d
    P = -(-K // w)
    Z = np.zeros((n, nc))
    X = None
    for p in range(P):
        k0, k1 = p * w, min((p + 1) * w, K)
        Us = U[k0 * d:k1 * d]
        rhs = Us.T if (p > 0 or B is None) else np.hstack([B, Us.T])
        sol = solve(A, rhs)
        if p == 0 and B is not None:
            X = sol[:, :B.shape[1]].copy()
            sol = sol[:, B.shape[1]:]
        Z[:, k0 * d:k1 * d] = sol             # k_mg_keep_z: the slice's columns of every state
    UZ = U @ Z
    M = np.eye(nc) + 0.5 * (UZ + UZ.T)
    Minv = solve(M, np.eye(nc))
    Minv = 0.5 * (Minv + Minv.T)
    Sxx = _ld(solve(A, np.eye(n))) - _ld(Z) @ _ld(Minv) @ _ld(Z).T
    if B is None:
        return Sxx.astype(np.float64), None, None, P
    Y = -Minv @ (U @ X)
    W = X + solve(A, U.T @ Y)                 # the final pass and k_clo_add
    Sl = solve(HLL - B.T @ W, np.eye(B.shape[1]))
    Sl = 0.5 * (Sl + Sl.T)
    return (Sxx + _ld(W) @ _ld(Sl) @ _ld(W).T).astype(np.float64), Sl, -W @ Sl, P
