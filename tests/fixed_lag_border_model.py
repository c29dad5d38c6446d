"""numpy model of fixed-lag smoothing with landmarks (gpslam_hip_marginalize_head_onto_landmarks, gpslam_hip_add_border_gaussians;
DESIGN.md section 4h): the head's Gaussian over the oldest kept state AND the landmarks.

The oracle cannot express a joint Gaussian on (x_i, v_i, l_0 .. l_{L-1}), so the reference of the device tests is the oracle's
normal_equations() -- all six arrays D, O, g, B, H_LL, g_L -- plus this file:
  border_problem  the test graphs: tests/test_gpu_fixed_lag.problem's well-conditioned chain plus landmarks, two ranges per interval
                  and landmark priors
  apply           a problem description onto a solver (gpslam_amd.synthetic.apply plus the plain range factors)
  head_tail       the description cut into the head's chain (states 0 .. k, every factor that touches a state < k, the landmarks'
                  positions, NO landmark priors) and the tail's (states k .., the rest, the landmark priors)
  schur_border    min over delta_0 .. delta_{k-1} of the head's quadratic by the border recursion, in float64 or longdouble
  schur_border_dense  the same through a dense solve (the check of the recursion)
  factor          fixed_lag_model.factor: it works at any size
  residual        r = A [Local(pose_lin, pose) ; vel - vel_lin ; l - lm_lin] - c through oracle.local
  step            one dense Gauss-Newton / damped step of a tail oracle chain that carries border Gaussians
  dense_marginals the dense inverse of the same system (the reference of the marginals)
"""
import numpy as np

from gpslam_amd import synthetic as S
from oracle import oracle as O
import fixed_lag_model as FL

FACTOR_KEYS = dict(FL.FACTOR_KEYS)
FACTOR_KEYS["prange_idx"] = (["prange_lm", "prange_z", "prange_sigma"], False)
LD = {O.POSE2: 2, O.POSE3: 3, O.LINEAR3: 2}


def positions(kind, pose):
    pose = np.asarray(pose)
    if kind == O.POSE3:
        return pose[..., 9:12]
    return pose[..., :2]


def border_problem(name, N, k, L, seed=5, priors=True, lpriors=True, plain=True):
    """problem(name, N, k)'s chain (sigma 0.05 / 0.1) plus L landmarks, two ranges per interval (sigma 0.1; an interpolated one and,
    with `plain`, a plain one on the interval's left state -- else two interpolated ones) and landmark priors (sigma 0.5).  Landmark 0
    is seen only from the head (states < k; at least from state 0), landmark 1 only from the tail (k = N - 1 leaves it to its prior),
    landmark 2 by the interpolated factor on (k - 1, k) -- and by whatever else the rotation gives it.  priors=False: no pose / velocity prior and no odometry (a gauge-free head)."""
    from test_gpu_fixed_lag import problem
    p = dict(problem(name, N, k))
    kind = p["kind"]
    ld = LD[kind]
    rng = np.random.default_rng(seed + 31 * L)
    if not priors:
        p = {key: v for key, v in p.items() if not key.startswith(("prior_", "vprior", "between_", "gps_"))}
    xy = positions(kind, p["pose"])
    lm = xy.mean(0) + 4.0 * rng.standard_normal((L, ld))
    left, which, tau = [], [], []
    pidx, pwhich = [], []

    def pick(i, j):
        """landmark of the j-th range of interval i: 0 only in the head, 1 only in the tail, 2 on (k - 1, k); the others in turn"""
        if i == k - 1 and j == 0:
            return 2
        if i == 0 and j == 1:
            return 0
        c = (2 * i + j) % L
        if c == 0 and i >= k:
            c = 3 % L if L > 3 else 2
        if c == 1 and i < k:
            c = 3 % L if L > 3 else 2
        return c

    for i in range(N - 1):
        left.append(i); which.append(pick(i, 0)); tau.append(0.4)
        if plain:
            pidx.append(i); pwhich.append(pick(i, 1))
        else:
            left.append(i); which.append(pick(i, 1)); tau.append(0.7)
    left, which, tau = np.array(left, dtype=np.int32), np.array(which, dtype=np.int32), np.array(tau)
    dt = p["gp_dt"][left]
    mid = xy[left] + (tau * 1.0)[:, None] * (xy[left + 1] - xy[left])
    p.update(landmarks=lm + 0.1 * rng.standard_normal((L, ld)), range_left=left, range_lm=which,
             range_z=np.linalg.norm(lm[which] - mid, axis=1) + 0.05 * rng.standard_normal(len(left)),
             range_sigma=np.full(len(left), 0.1), range_dt=dt, range_tau=tau * dt)
    if plain:
        pidx, pwhich = np.array(pidx, dtype=np.int32), np.array(pwhich, dtype=np.int32)
        p.update(prange_idx=pidx, prange_lm=pwhich, prange_z=np.linalg.norm(lm[pwhich] - xy[pidx], axis=1) + 0.05 * rng.standard_normal(len(pidx)),
                 prange_sigma=np.full(len(pidx), 0.1))
    if lpriors:
        p.update(lprior_idx=np.arange(L, dtype=np.int32), lprior=lm.copy(), lprior_sig=np.full((L, ld), 0.5))
    return p


def apply(p, solver):
    S.apply(p, solver)
    if "prange_idx" in p and len(p["prange_idx"]):
        solver.add_range(p["prange_idx"], p["prange_lm"], p["prange_z"], p["prange_sigma"])
        solver.compile()
    return solver


def chain(p, **kw):
    return O.Chain(p["kind"], landmark_dim=LD[p["kind"]] if "landmarks" in p else 0, **kw)


def head_tail(p, k):
    N = p["pose"].shape[0]
    head = dict(kind=p["kind"], qc=p["qc"], N=k + 1, pose=p["pose"][:k + 1].copy(), vel=p["vel"][:k + 1].copy(), landmarks=p["landmarks"])
    tail = dict(kind=p["kind"], qc=p["qc"], N=N - k, pose=p["pose"][k:].copy(), vel=p["vel"][k:].copy())
    for key in ("landmarks", "lprior_idx", "lprior", "lprior_sig"):
        if key in p:
            tail[key] = p[key]
    for key, (others, _two) in FACTOR_KEYS.items():
        if key not in p:
            continue
        idx = np.asarray(p[key])
        m = idx < k
        head[key] = idx[m].astype(np.int32)
        tail[key] = (idx[~m] - k).astype(np.int32)
        for o in others:
            head[o] = np.asarray(p[o])[m]
            tail[o] = np.asarray(p[o])[~m]
    return head, tail


def head_arrays(p, k):
    head, _ = head_tail(p, k)
    return apply(head, chain(head)).normal_equations()


def schur_border(D, Om, g, B, HLL, gL, k, dtype=np.float64):
    """(Lambda, gamma, scale, gscale) over (delta_k, delta_l): the arrays of the head chain of head_tail (block k and H_LL hold the
    head's share only); scale = max |diag| of [D_k ; H_LL] before the subtraction, gscale = max |g|, |g_L|."""
    D, Om, g, B, HLL, gL = (a.astype(dtype) for a in (D, Om, g, B, HLL, gL))
    nl = HLL.shape[0]
    G = lambda i: np.concatenate([g[i][:, None], B[i]], axis=1)
    Sx, Gx, T = D[0].copy(), G(0), np.zeros((1 + nl, 1 + nl), dtype=dtype)
    for i in range(k):
        L = FL._chol(Sx)
        V = FL._fwd(L, Om[i].T)
        W = FL._fwd(L, Gx)
        Sx = D[i + 1] - V.T @ V
        Gx = G(i + 1) - V.T @ W
        T = T + W.T @ W
    Lam = np.block([[Sx, Gx[:, 1:]], [Gx[:, 1:].T, HLL - T[1:, 1:]]])
    vec = np.concatenate([Gx[:, 0], gL - T[1:, 0]])
    scale = float(max(np.abs(np.diag(D[k])).max(), np.abs(np.diag(HLL)).max()))
    return Lam, -vec, scale, float(max(np.abs(g).max(), np.abs(gL).max()))


def dense_system(D, Om, g, B, HLL, gL):
    """H, rhs over [x_0 .. x_{N-1} ; l] in the records' convention (rhs = -J^T e)"""
    N, b = g.shape
    nl = HLL.shape[0]
    H = np.zeros((N * b + nl, N * b + nl))
    H[:N * b, :N * b] = FL.dense(D, Om)
    H[:N * b, N * b:] = B.reshape(N * b, nl)
    H[N * b:, :N * b] = B.reshape(N * b, nl).T
    H[N * b:, N * b:] = HLL
    return H, np.concatenate([g.reshape(-1), gL])


def schur_border_dense(D, Om, g, B, HLL, gL, k):
    b = D.shape[1]
    H, rhs = dense_system(D[:k + 1], Om[:k + 1], g[:k + 1], B[:k + 1], HLL, gL)
    n = k * b
    Hhh, Hkh, Hkk = H[:n, :n], H[n:, :n], H[n:, n:]
    X = np.linalg.solve(Hhh, np.concatenate([Hkh.T, rhs[:n, None]], 1))
    return Hkk - Hkh @ X[:, :-1], -(rhs[n:] - Hkh @ X[:, -1])


factor = FL.factor


def xi_of(kind, chart, pose_lin, vel_lin, lm_lin, pose, vel, lm):
    return np.concatenate([O.local(kind, pose_lin, pose, chart), np.asarray(vel) - np.asarray(vel_lin),
                           (np.asarray(lm) - np.asarray(lm_lin)).reshape(-1)])


def residual(kind, chart, pose_lin, vel_lin, lm_lin, A, c, pose, vel, lm):
    return A @ xi_of(kind, chart, pose_lin, vel_lin, lm_lin, pose, vel, lm) - c


def system(orc, kind, chart, gaussians):
    """(H, rhs, err): the dense normal equations of the oracle chain `orc` (the tail's factors) plus border Gaussians
    (idx, pose_lin, vel_lin, lm_lin, A, c): A^T A on the columns of state idx and of the landmarks, A^T (c - A xi) on the right-hand
    side; err the graph error, the oracle's plus |r|^2 / 2 of each."""
    pose, vel = orc.get_states()
    lm = orc.get_landmarks()
    H, rhs = dense_system(*orc.normal_equations())
    N, b = pose.shape[0], 2 * O.TANGENT_DIM[kind]
    err = orc.error()
    for idx, pl, vl, ll, A, c in gaussians:
        xi = xi_of(kind, chart, pl, vl, ll, pose[idx], vel[idx], lm)
        cols = np.concatenate([np.arange(idx * b, (idx + 1) * b), np.arange(N * b, H.shape[0])])
        H[np.ix_(cols, cols)] += A.T @ A
        rhs[cols] += A.T @ (c - A @ xi)
        r = A @ xi - c
        err += 0.5 * float(r @ r)
    return H, rhs, err


def step(orc, kind, chart, gaussians, lam=0.0):
    """One Gauss-Newton (lam = 0) or damped (H + lam I) step; returns (pose, vel, landmarks, error after) and leaves them in orc."""
    pose, vel = orc.get_states()
    lm = orc.get_landmarks()
    H, rhs, _ = system(orc, kind, chart, gaussians)
    N, d = pose.shape[0], O.TANGENT_DIM[kind]
    b = 2 * d
    delta = np.linalg.solve(H + lam * np.eye(H.shape[0]), rhs)
    x = delta[:N * b].reshape(N, b)
    pose = np.stack([O.retract(kind, pose[i], x[i, :d], chart) for i in range(N)])
    vel = vel + x[:, d:]
    lm = lm + delta[N * b:].reshape(lm.shape)
    orc.set_states(pose, vel)
    orc.set_landmarks(lm)
    return pose, vel, lm, system(orc, kind, chart, gaussians)[2]


def dense_marginals(orc, kind, chart, gaussians):
    H, _, _ = system(orc, kind, chart, gaussians)
    return np.linalg.inv(H)
