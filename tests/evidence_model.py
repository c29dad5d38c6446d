"""numpy model of gpslam_hip_log_determinant (gpslam_amd/csrc/evidence.hip): the forward half of the chunked elimination of a
block-tridiagonal SPD matrix with the logarithms of its pivots summed (marginals_model.selinv's forward half plus the sums), the
low-rank parts of loop closures and landmarks, the noise models' normaliser, and the textbook marginal likelihood of a linear GP
regression, which the Laplace log-evidence equals on a graph whose factors are all linear."""
import numpy as np

CHUNK = 16   # kMgChunk
LOG_2PI = float(np.log(2.0 * np.pi))


def logdet_tol(H):
    """Absolute bound on the error of a computed log det H.  From d log det H = tr(H^-1 dH), a relative perturbation eps of H's
    entries moves log det H by at most n eps kappa; the bound is n * 100 EPS kappa with kappa the condition number of the
    Jacobi-scaled H (as the marginals' tol_of computes it, with its cap kappa <= 1e9), floored at n * 1e-13."""
    s = np.sqrt(np.diag(H))
    kappa = np.linalg.cond(H / np.outer(s, s))
    assert kappa <= 1e9, kappa
    n = H.shape[0]
    return max(n * 1e-13, n * 100 * np.finfo(float).eps * kappa)


def reference_logdet(H):
    """(slogdet's log det H, the bound): the reference side of every comparison, itself held to the bound against the Cholesky
    factor's pivots, so that the bound is shown to hold for the reference alone."""
    tol = logdet_tol(H)
    sign, ref = np.linalg.slogdet(H)
    assert sign == 1.0
    chol = 2.0 * float(np.sum(np.log(np.diag(np.linalg.cholesky(H)))))
    assert abs(ref - chol) <= tol, (ref, chol, tol)
    return float(ref), tol


def banded_reference_logdet(D, O, iters=30):
    """(log det, the bound) of a block-tridiagonal matrix too large for a dense reference: log det by the plain block recursion
    P_{i+1} = D_{i+1} - O_i P_i^-1 O_i^T (no chunks, another order of operations than the device's), kappa of the Jacobi-scaled
    matrix from power iterations -- lambda_max by products, 1 / lambda_min by solves with the same recursion.  Power iteration
    approaches either from inside the spectrum, so kappa is if anything underestimated and the bound tighter than logdet_tol's."""
    N, b = D.shape[0], D.shape[1]
    s = np.sqrt(np.einsum("nii->ni", D))
    Ds = D / (s[:, :, None] * s[:, None, :])
    Os = np.zeros_like(O)
    Os[:-1] = O[:-1] / (s[1:, :, None] * s[:-1, None, :])
    P, G = np.zeros_like(Ds), np.zeros_like(Ds)
    P[0] = Ds[0]
    logdet = 0.0
    for i in range(N):
        L = np.linalg.cholesky(P[i])
        logdet += 2.0 * float(np.sum(np.log(np.diag(L))))
        if i + 1 < N:
            G[i] = np.linalg.solve(P[i], Os[i].T).T            # O_i P_i^-1
            P[i + 1] = Ds[i + 1] - G[i] @ Os[i].T
    logdet += 2.0 * float(np.sum(np.log(s)))                   # det H = det(S)^2 det(H scaled)
    Pinv = np.linalg.inv(P)

    def matvec(x):
        y = np.einsum("nij,nj->ni", Ds, x)
        y[1:] += np.einsum("nij,nj->ni", Os[:-1], x[:-1])
        y[:-1] += np.einsum("nji,nj->ni", Os[:-1], x[1:])
        return y

    def solve(r):
        y = r.copy()
        for i in range(N - 1):
            y[i + 1] -= G[i] @ y[i]
        x = np.zeros_like(y)
        x[N - 1] = Pinv[N - 1] @ y[N - 1]
        for i in range(N - 2, -1, -1):
            x[i] = Pinv[i] @ (y[i] - Os[i].T @ x[i + 1])
        return x

    rng = np.random.default_rng(0)
    u, v = rng.standard_normal((N, b)), rng.standard_normal((N, b))
    lmax = linv = 0.0
    for _ in range(iters):
        u /= np.linalg.norm(u); v /= np.linalg.norm(v)
        u2, v2 = matvec(u), solve(v)
        lmax, linv = float(np.sum(u * u2)), float(np.sum(v * v2))
        u, v = u2, v2
    kappa = lmax * linv
    assert kappa <= 1e9, kappa
    n = N * b
    return logdet, max(n * 1e-13, n * 100 * np.finfo(float).eps * kappa)


def chain_logdet(D, O, C=CHUNK):
    """log det of the block-tridiagonal matrix (D, O[i] = A_{i+1,i}) by the recursion of k_ev_forward / k_ev_top: per interior state
    one Cholesky factor L of the pivot block, E^ = L^-1 E, F^ = L^-1 F, every Schur update a product of those two; nothing kept
    but the separators' system and the sum of log-pivots.  Returns (log det, number of levels above 0)."""
    N, b = D.shape[0], D.shape[1]
    if N == 1:
        return 2.0 * float(np.sum(np.log(np.diag(np.linalg.cholesky(D[0]))))), 0
    E = [O[i].T if i + 1 < N else np.zeros((b, b)) for i in range(N)]     # E_i = A_{i,i+1}
    nu = -(-N // C)
    upD, upO, add = np.zeros((nu, b, b)), np.zeros((nu, b, b)), np.zeros((nu, b, b))
    total = 0.0
    for k in range(nu):
        s, e = k * C, min(k * C + C, N)
        right = e < N
        Ds = D[s].copy()
        part = 0.0
        if e == s + 1:
            upD[k], upO[k] = Ds, (O[s] if right else 0.0)
            continue
        P, F = D[s + 1].copy(), O[s].copy()
        for j in range(s + 1, e):
            L = np.linalg.cholesky(P)
            part += 2.0 * float(np.sum(np.log(np.diag(L))))
            EF = np.linalg.solve(L, np.hstack([E[j], F]))        # (one forward substitution on [E | F])
            Eh, Fh = EF[:, :b], EF[:, b:]
            Ds -= Fh.T @ Fh
            if j + 1 < e:
                P, F = D[j + 1] - Eh.T @ Eh, -Eh.T @ Fh
            else:
                if right:
                    add[k + 1] = Eh.T @ Eh
                upO[k] = -Eh.T @ Fh
        upD[k] = Ds
        total += part
    upper, levels = chain_logdet(upD - add, upO, C)
    return total + upper, levels + 1


def lowrank_parts(Ainv, B, Jc, HLL):
    """(log det(I + U Z), log det S) with M and S as marginals_model.lowrank forms them: Z = A^-1 Jc^T, M = I + Jc Z,
    S = HLL - B^T (A + Jc^T Jc)^-1 B."""
    n = Ainv.shape[0]
    Z = Ainv @ Jc.T if Jc is not None else np.zeros((n, 0))
    M = np.eye(Z.shape[1]) + (Jc @ Z if Jc is not None else 0.0)
    ld_m = float(np.linalg.slogdet(0.5 * (M + M.T))[1]) if Z.shape[1] else 0.0
    if B is None or B.shape[1] == 0:
        return ld_m, 0.0
    Hxx_inv = Ainv - Z @ np.linalg.inv(M) @ Z.T
    S = HLL - B.T @ Hxx_inv @ B
    return ld_m, float(np.linalg.slogdet(S)[1])


def gp_Q(dt, Qc):
    return np.block([[dt ** 3 / 3 * Qc, dt ** 2 / 2 * Qc], [dt ** 2 / 2 * Qc, dt * Qc]])


def gp_Phi(dt, d):
    return np.block([[np.eye(d), dt * np.eye(d)], [np.zeros((d, d)), np.eye(d)]])


def gp_log_normaliser(Qc, dt):
    """log|det R| of one GP prior: -1/2 (d log(dt^4 / 12) + 2 log det Qc)"""
    d = Qc.shape[0]
    return -0.5 * (d * (4.0 * np.log(dt) - np.log(12.0)) + 2.0 * float(np.linalg.slogdet(Qc)[1]))


def combine(cost, logdet, lognorm, rows, nvars):
    return -cost + lognorm - 0.5 * logdet - 0.5 * (rows - nvars) * LOG_2PI


def gp_prior_moments(m0, P0, dts, Qc):
    """Mean and covariance of the whole trajectory [x_0; ...; x_{N-1}], x = [position; velocity], of the white-noise-on-acceleration
    prior: x_0 ~ N(m0, P0), x_{i+1} = Phi(dt_i) x_i + w_i, w_i ~ N(0, Q(dt_i)).  No Jacobian and no information matrix is formed."""
    d = Qc.shape[0]
    b = 2 * d
    N = len(dts) + 1
    mean = np.zeros(N * b)
    K = np.zeros((N * b, N * b))
    mean[:b] = m0
    K[:b, :b] = P0
    for i in range(N - 1):
        Phi, Q = gp_Phi(dts[i], d), gp_Q(dts[i], Qc)
        r0, r1 = slice(i * b, (i + 1) * b), slice((i + 1) * b, (i + 2) * b)
        mean[r1] = Phi @ mean[r0]
        K[r1, :(i + 1) * b] = Phi @ K[r0, :(i + 1) * b]           # cov(x_{i+1}, x_j) = Phi cov(x_i, x_j), j <= i
        K[:(i + 1) * b, r1] = K[r1, :(i + 1) * b].T
        K[r1, r1] = Phi @ K[r0, r0] @ Phi.T + Q
    return mean, K


def gp_marginal_loglik(m0, P0, dts, Qc, meas_idx, y, sig):
    """log N(y; C m, C K C^T + R): the marginal likelihood of position measurements y (len(meas_idx) x d, sigmas sig of the same
    shape) of the states meas_idx under the GP prior above -- the textbook GP-regression evidence."""
    d = Qc.shape[0]
    b = 2 * d
    mean, K = gp_prior_moments(m0, P0, dts, Qc)
    rows = np.concatenate([np.arange(i * b, i * b + d) for i in meas_idx])
    Sy = K[np.ix_(rows, rows)] + np.diag(np.asarray(sig, dtype=float).reshape(-1) ** 2)
    r = np.asarray(y, dtype=float).reshape(-1) - mean[rows]
    L = np.linalg.cholesky(Sy)
    a = np.linalg.solve(L, r)
    return -0.5 * float(a @ a) - float(np.sum(np.log(np.diag(L)))) - 0.5 * len(r) * LOG_2PI


def linear_gp_problem(N=40, d=3, dt=0.1, theta=1.0, every=4, seed=0):
    """The linear test problem of the evidence: a trajectory drawn from the GP at theta * Qc0, position measurements of every
    `every`-th state.  Returns a dict with everything both the model and a solver need."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((d, d))
    Qc0 = G @ G.T / d + np.eye(d)
    m0 = np.concatenate([rng.standard_normal(d), 0.5 * rng.standard_normal(d)])
    sp, sv = np.full(d, 0.2), np.full(d, 0.3)
    P0 = np.diag(np.concatenate([sp, sv]) ** 2)
    dts = np.full(N - 1, dt)
    x = np.zeros((N, 2 * d))
    x[0] = m0 + np.sqrt(np.diag(P0)) * rng.standard_normal(2 * d)
    for i in range(N - 1):
        Lq = np.linalg.cholesky(gp_Q(dts[i], theta * Qc0))
        x[i + 1] = gp_Phi(dts[i], d) @ x[i] + Lq @ rng.standard_normal(2 * d)
    meas_idx = np.arange(every - 1, N, every, dtype=np.int32)
    sig = np.full((len(meas_idx), d), 0.05)
    y = x[meas_idx, :d] + sig * rng.standard_normal(sig.shape)
    return dict(N=N, d=d, Qc0=Qc0, m0=m0, P0=P0, sp=sp, sv=sv, dts=dts, meas_idx=meas_idx, y=y, sig=sig, x=x)


def linear_gp_graph_logZ(pr, theta):
    """The same evidence through the Laplace formula on the DENSE least-squares problem (exact: every factor is linear): builds J
    and the right-hand side, solves, and combines.  Returns (log Z, cost at the optimum, log det H, lognorm, m - n)."""
    N, d = pr["N"], pr["d"]
    b = 2 * d
    Qc = theta * pr["Qc0"]
    rows, rhs = [], []
    W0 = np.diag(1.0 / np.sqrt(np.diag(pr["P0"])))
    J = np.zeros((b, N * b)); J[:, :b] = W0
    rows.append(J); rhs.append(W0 @ pr["m0"])
    lognorm = float(np.sum(np.log(np.diag(W0))))
    for i in range(N - 1):
        Rq = np.linalg.cholesky(np.linalg.inv(gp_Q(pr["dts"][i], Qc))).T
        J = np.zeros((b, N * b))
        J[:, i * b:(i + 1) * b] = -Rq @ gp_Phi(pr["dts"][i], d)
        J[:, (i + 1) * b:(i + 2) * b] = Rq
        rows.append(J); rhs.append(np.zeros(b))
        lognorm += gp_log_normaliser(Qc, pr["dts"][i])
    for k, i in enumerate(pr["meas_idx"]):
        J = np.zeros((d, N * b))
        J[:, i * b:i * b + d] = np.diag(1.0 / pr["sig"][k])
        rows.append(J); rhs.append(pr["y"][k] / pr["sig"][k])
        lognorm -= float(np.sum(np.log(pr["sig"][k])))
    J, r = np.vstack(rows), np.concatenate(rhs)
    H = J.T @ J
    xh = np.linalg.solve(H, J.T @ r)
    cost = 0.5 * float(np.sum((J @ xh - r) ** 2))
    logdet = float(np.linalg.slogdet(H)[1])
    m, n = J.shape
    return combine(cost, logdet, lognorm, m, n), cost, logdet, lognorm, m - n
