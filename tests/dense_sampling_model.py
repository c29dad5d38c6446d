"""Posterior sampling at query times (include/gpslam_hip_sampling_at.h) in plain numpy: the reference side of
tests/test_dense_sampling_model.py and tests/test_gpu_sampling_at.py.

Inside interval i the interpolators work in the local variable of the left state, gamma(t) = [xi(t); xi'(t)], xi = Log(T_i^-1 T(t)),
where the prior is the linear white-noise-on-acceleration process: Phi(t) = [[1, t], [0, 1]], Q(t) = [[t^3/3, t^2/2], [t^2/2, t]] (x) Qc.

The walk (the interface's formula, one query after the other):
  bridge        Lambda, Psi, K and the closed-form Cholesky factor l of K for times a < tau < b, as 2 x 2 matrices (Qc cancels or factors out)
  walk_weights  the walk as a linear map: gamma_k = A_k gamma(0) + B_k gamma(dt) + sum_j N_kj eps_j, in 2 x 2 blocks
  ends          gamma(0) and gamma(dt) of an interval from oracle primitives only (oracle.local; oracle.gp_prior for J v_2)
  walk          the draw of one run: poses T_i (+) Exp(xi_k) (oracle.retract, expmap chart) and the gamma_k

An independent route to the same law:
  conditioning  mean weights and joint covariance of gamma(tau_1 .. tau_m) given both ends, by direct Gaussian conditioning of the
                prior kernel Cov(gamma(s), gamma(t)) = Q(s) Phi(t - s)^T (s <= t), in full dimension with Qc inside

Helpers of the device tests:
  runs          the runs of equal `left` of a query list
  noise_index   where query q's normals sit in a noise vector
  linear_maps   on a vector space: G (queries from the stacked support states) and the bridge's joint covariance, per call
"""
import numpy as np

from oracle import oracle as O

VECTOR = (O.LINEAR2, O.LINEAR3)


def phi(t):
    return np.array([[1.0, t], [0.0, 1.0]])


def q2(t):
    return np.array([[t ** 3 / 3.0, t ** 2 / 2.0], [t ** 2 / 2.0, t]])


def bridge(a, tau, b):
    """(Lambda, Psi, K, l) of gamma(tau) | gamma(a), gamma(b), each 2 x 2: Psi = Q(u) Phi(s)^T Q(T)^-1, Lambda = Phi(u) - Psi Phi(T) from
    the matrices; K and its lower Cholesky factor l in the closed forms of the header"""
    u, s = tau - a, b - tau
    T = u + s
    Psi = q2(u) @ phi(s).T @ np.linalg.inv(q2(T))
    Lam = phi(u) - Psi @ phi(T)
    K = np.array([[u ** 3 * s ** 3 / 3.0, u ** 2 * s ** 2 * (s - u) / 2.0],
                  [u ** 2 * s ** 2 * (s - u) / 2.0, u * s * (s * s - s * u + u * u)]]) / T ** 3
    l = np.array([[(u * s) ** 1.5 / np.sqrt(3.0 * T ** 3), 0.0],
                  [np.sqrt(3.0) * (s - u) * np.sqrt(u * s) / (2.0 * T ** 1.5), 0.5 * np.sqrt(u * s / T)]])
    return Lam, Psi, K, l


def walk_weights(dt, taus):
    """(A (m, 2, 2), B (m, 2, 2), N (2m, 2m)): gamma_k = A_k gamma(0) + B_k gamma(dt) + (N (x) L_q) eps restricted to rows of query k, eps
    ordered per query [eps_p; eps_v]"""
    m = len(taus)
    A, B, N = np.zeros((m, 2, 2)), np.zeros((m, 2, 2)), np.zeros((2 * m, 2 * m))
    Ap, Bp, Np, a = np.eye(2), np.zeros((2, 2)), np.zeros((2, 2 * m)), 0.0
    for k, tau in enumerate(taus):
        Lam, Psi, _, l = bridge(a, tau, dt)
        Ap, Bp, Np = Lam @ Ap, Lam @ Bp + Psi, Lam @ Np
        Np[:, 2 * k:2 * k + 2] += l
        A[k], B[k], N[2 * k:2 * k + 2] = Ap, Bp, Np
        a = tau
    return A, B, N


def conditioning(dt, taus, Qc):
    """(Wa, Wb, C): E gamma(taus) = Wa gamma(0) + Wb gamma(dt) and Cov = C, all in full dimension (2 d m rows, per query [xi; xi']), by
    conditioning the process started at gamma(0) -- gamma(t) = Phi(t) gamma(0) + w(t), Cov(w(s), w(t)) = Q(s) Phi(t - s)^T -- on gamma(dt)"""
    Qc = np.asarray(Qc, dtype=np.float64)
    d = Qc.shape[0]
    I = np.eye(d)
    ts = list(taus) + [dt]
    n = len(ts)
    S = np.zeros((2 * d * n, 2 * d * n))
    for i, s in enumerate(ts):
        for j, t in enumerate(ts):
            blk = np.kron(q2(s) @ phi(t - s).T, Qc) if s <= t else np.kron(phi(s - t) @ q2(t), Qc)
            S[2 * d * i:2 * d * (i + 1), 2 * d * j:2 * d * (j + 1)] = blk
    m = 2 * d * (n - 1)
    Sqq, Sqb, Sbb = S[:m, :m], S[:m, m:], S[m:, m:]
    Wb = np.linalg.solve(Sbb, Sqb.T).T
    Wa = np.concatenate([np.kron(phi(t), I) for t in taus]) - Wb @ np.kron(phi(dt), I)
    return Wa, Wb, Sqq - Wb @ Sqb.T


def full(blocks, M):
    """the 2 x 2-block form (m, 2, 2) (x) M stacked: (2 d m, 2 d)"""
    return np.concatenate([np.kron(b, M) for b in blocks])


def ends(kind, p1, v1, p2, v2, dt):
    """(gamma(0), gamma(dt)) = ([0; v_1], [xi_12; J v_2]) of one interval: xi_12 by oracle.local under the expmap chart, J v_2 from the
    velocity half of the oracle's GP prior error -- v_1 - v_2 on the vector spaces (its error there is dt v_1 - (p_2 - p_1), v_1 - v_2),
    J v_2 - v_1 on the groups (J = Jr^-1(xi_12) on SE(3), I on SE(2) and SO(3), as the reference's interpolators have it)"""
    d = O.TANGENT_DIM[kind]
    v1 = np.asarray(v1, dtype=np.float64)
    e, _ = O.gp_prior(kind, p1, v1, p2, v2, dt, jac=False)
    jv2 = v1 - e[d:] if kind in VECTOR else e[d:] + v1
    return np.concatenate([np.zeros(d), v1]), np.concatenate([O.local(kind, p1, p2, O.CHART_EXPMAP), jv2])


def walk(kind, p1, v1, p2, v2, dt, taus, Lq, eps):
    """the draw of one run: (poses (m, pose_dim), gammas (m, 2 d)); eps (m, 2 d), per query [eps_p; eps_v]; Lq the lower Cholesky factor
    of Qc"""
    d = O.TANGENT_DIM[kind]
    I = np.eye(d)
    g, gb = ends(kind, p1, v1, p2, v2, dt)
    eps = np.asarray(eps, dtype=np.float64).reshape(len(taus), 2 * d)
    poses, gammas, a = [], [], 0.0
    for k, tau in enumerate(taus):
        Lam, Psi, _, l = bridge(a, tau, dt)
        wp, wv = Lq @ eps[k, :d], Lq @ eps[k, d:]
        g = np.kron(Lam, I) @ g + np.kron(Psi, I) @ gb + np.concatenate([l[0, 0] * wp, l[1, 0] * wp + l[1, 1] * wv])
        poses.append(O.retract(kind, p1, g[:d], O.CHART_EXPMAP))
        gammas.append(g)
        a = tau
    return np.stack(poses), np.stack(gammas)


def runs(left):
    """[(first query, one past the last)] of the runs of equal left"""
    left = np.asarray(left)
    cut = [0] + [q for q in range(1, len(left)) if left[q] != left[q - 1]] + [len(left)]
    return list(zip(cut[:-1], cut[1:]))


def noise_index(n_noise, d, q):
    """the 2 d noise indices of query q: eps_p, then eps_v"""
    return n_noise + 2 * d * q + np.arange(2 * d)


def walk_call(kind, poses, vels, left, dt, tau, Lq, eps):
    """a whole call's queries from one draw's support states: (query poses (n, pose_dim), gammas (n, 2 d)); eps (n, 2 d)"""
    d = O.TANGENT_DIM[kind]
    eps = np.asarray(eps, dtype=np.float64).reshape(len(left), 2 * d)
    P, G = [], []
    for q0, q1 in runs(left):
        i = int(left[q0])
        p, g = walk(kind, poses[i], vels[i], poses[i + 1], vels[i + 1], float(dt[q0]), [float(t) for t in tau[q0:q1]], Lq, eps[q0:q1])
        P.append(p)
        G.append(g)
    return np.concatenate(P), np.concatenate(G)


def linear_maps(N, d, left, dt, tau, Qc):
    """On a vector space, with x = the stacked states [p_0; v_0; p_1; v_1; ...] (N * 2 d): (G, C) with
    [p(tau_q); v(tau_q)] stacked over the queries (n * 2 d) = G x + noise of covariance C.  G from the walk's weights (p(tau) =
    p_i + xi(tau), xi(dt) = p_i+1 - p_i), C block-diagonal over the runs, each block from the conditioning route."""
    n = len(left)
    G, Cc = np.zeros((2 * d * n, 2 * d * N)), np.zeros((2 * d * n, 2 * d * n))
    I = np.eye(d)
    for q0, q1 in runs(left):
        i = int(left[q0])
        taus = [float(t) for t in tau[q0:q1]]
        A, B, _ = walk_weights(float(dt[q0]), taus)
        for k in range(q1 - q0):
            r = 2 * d * (q0 + k)
            rows = G[r:r + 2 * d]
            ci, cj = 2 * d * i, 2 * d * (i + 1)
            rows[:, ci:ci + 2 * d] += np.kron(A[k], I)             # gamma(0) = [0; v_i]: the position column meets a zero ...
            rows[:, ci:ci + d] = 0.0
            rows[:, cj:cj + 2 * d] += np.kron(B[k], I)             # gamma(dt) = [p_i+1 - p_i; v_i+1]
            rows[:, ci:ci + d] -= np.kron(B[k][:, :1], I)
            rows[:d, ci:ci + d] += I                               # p = p_i + xi
        _, _, C = conditioning(float(dt[q0]), taus, Qc)
        Cc[2 * d * q0:2 * d * q1, 2 * d * q0:2 * d * q1] = C
    return G, Cc
