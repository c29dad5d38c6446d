"""numpy model of gpslam_hip_marginals (gpslam_amd/csrc/marginals.hip): the chunked selected inversion of a block-tridiagonal
SPD matrix, the low-rank term of landmarks and loop closures, and the GP term of the interpolated covariance."""
import numpy as np

CHUNK = 16   # kMgChunk


def dense(D, O):
    """The block-tridiagonal matrix of diagonal blocks D and O[i] = A_{i+1,i} (gpslam_hip_normal_equations' convention)."""
    N, b = D.shape[0], D.shape[1]
    A = np.zeros((N * b, N * b))
    for i in range(N):
        A[i * b:(i + 1) * b, i * b:(i + 1) * b] = D[i]
        if i + 1 < N:
            A[(i + 1) * b:(i + 2) * b, i * b:(i + 1) * b] = O[i]
            A[i * b:(i + 1) * b, (i + 1) * b:(i + 2) * b] = O[i].T
    return A


def selinv(D, O, C=CHUNK):
    """Sigma_{i,i} and Sigma_{i,i+1} of A^-1 by the recursion of k_mg_forward / k_mg_top / k_mg_backward."""
    N, b = D.shape[0], D.shape[1]
    if N == 1:
        return np.linalg.inv(D), np.zeros_like(D)
    E = [O[i].T if i + 1 < N else np.zeros((b, b)) for i in range(N)]     # E_i = A_{i,i+1}
    nu = -(-N // C)
    upD, upO, add = np.zeros((nu, b, b)), np.zeros((nu, b, b)), np.zeros((nu, b, b))
    fac = {}
    for k in range(nu):
        s, e = k * C, min(k * C + C, N)
        right = e < N
        Ds = D[s].copy()
        if e == s + 1:
            upD[k], upO[k] = Ds, (O[s] if right else 0.0)
            continue
        P, F = D[s + 1].copy(), O[s].copy()
        for j in range(s + 1, e):
            Pi = np.linalg.inv(P)
            U, V = Pi @ E[j], Pi @ F
            fac[j] = (Pi, U, V)
            Ds -= F.T @ V
            if j + 1 < e:
                P, F = D[j + 1] - E[j].T @ U, -E[j].T @ V
            else:
                if right:
                    add[k + 1] = E[j].T @ U
                upO[k] = -E[j].T @ V
        upD[k] = Ds
    uSd, uSn = selinv(upD - add, upO, C)
    Sd, Sn = np.zeros((N, b, b)), np.zeros((N, b, b))
    for k in range(nu):
        s, e = k * C, min(k * C + C, N)
        right = e < N
        Sss = uSd[k]
        Sd[s] = Sss
        if e == s + 1:
            Sn[s] = uSn[k] if right else 0.0
            continue
        Snn = uSd[k + 1] if right else np.zeros((b, b))
        Sns = uSn[k].T if right else np.zeros((b, b))
        for j in range(e - 1, s, -1):
            Pi, U, V = fac[j]
            Sjs = -U @ Sns - V @ Sss
            Sjn = -U @ Snn - V @ Sns.T
            Sjj = Pi - U @ Sjn.T - V @ Sjs.T
            Sd[j], Sn[j] = Sjj, Sjn
            Sns, Snn = Sjs, Sjj
        Sn[s] = Sns.T
    return Sd, Sn


def lowrank(Ainv, B, Jc, HLL):
    """Sigma of [[A + Jc^T Jc, B], [B^T, HLL]] as A^-1 + Y K Y^T etc. (k_mg_core / k_mg_finish): returns (Sxx, SxL, SLL)."""
    n = Ainv.shape[0]
    nl = 0 if B is None else B.shape[1]
    Z = Ainv @ Jc.T if Jc is not None else np.zeros((n, 0))
    M = np.eye(Z.shape[1]) + (Jc @ Z if Jc is not None else 0.0)
    Minv = np.linalg.inv(M)
    Hxx_inv = Ainv - Z @ Minv @ Z.T
    if nl:
        W = Hxx_inv @ B                       # the landmark columns after the closure correction
        S = HLL - B.T @ W
        Sinv = np.linalg.inv(S)
    else:
        W, Sinv = np.zeros((n, 0)), np.zeros((0, 0))
    Y = np.hstack([W, Z])
    K = np.zeros((Y.shape[1], Y.shape[1]))
    K[:nl, :nl] = Sinv
    K[nl:, nl:] = -Minv
    return Ainv + Y @ K @ Y.T, -(Y @ K)[:, :nl], Sinv


def gp_c(dt, tau):
    """c(dt, tau): the pose block of Q(tau) - Psi Phi(dt - tau) Q(tau) is c * Qc."""
    return tau ** 3 * (dt - tau) ** 3 / (3.0 * dt ** 3)


def gp_conditional(dt, tau, Qc):
    """Q(tau) - Psi Phi(dt - tau) Q(tau) with Q, Phi, Psi of gpslam/gp/GPutils.h:24-71."""
    d = Qc.shape[0]

    def Q(t):
        return np.block([[t ** 3 / 3 * Qc, t ** 2 / 2 * Qc], [t ** 2 / 2 * Qc, t * Qc]])

    def Phi(t):
        return np.block([[np.eye(d), t * np.eye(d)], [np.zeros((d, d)), np.eye(d)]])

    Psi = Q(tau) @ Phi(dt - tau).T @ np.linalg.inv(Q(dt))
    return Q(tau) - Psi @ Phi(dt - tau) @ Q(tau)


def random_chain(N, b, seed=0):
    """A random SPD block-tridiagonal matrix (D, O), diagonally dominant enough to be well conditioned."""
    rng = np.random.default_rng(seed)
    D = np.zeros((N, b, b))
    O = 0.3 * rng.standard_normal((N, b, b))
    O[-1] = 0.0
    for i in range(N):
        G = rng.standard_normal((b, b))
        D[i] = G @ G.T / b + (2.0 + 2 * 0.3 * b) * np.eye(b)
    return D, O
