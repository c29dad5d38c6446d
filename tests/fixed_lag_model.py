"""numpy model of fixed-lag smoothing (gpslam_hip_marginalize_head, gpslam_hip_add_state_gaussians).

The oracle cannot express a joint Gaussian on (x_i, v_i), so the reference of the device tests is the oracle's arrays plus this file:
  head_tail      a problem description (gpslam_amd.synthetic format) cut into the head's chain (states 0 .. k, every factor that
                 touches a state < k) and the tail's (states k .., the rest, indices lowered by k)
  schur          min over delta_0 .. delta_{k-1} of the head's quadratic, by the block recursion D'_{i+1} = D_{i+1} - O_i D'_i^-1 O_i^T
                 on the oracle's normal_equations() of the head chain (O_i = H_{i+1,i}, g = -J^T e: the records' conventions)
  factor         Lambda = A^T A, A^T c = -gamma by Cholesky with diagonal pivoting, small pivots to zero rows
  residual       r = A [Local(pose_lin, pose) ; vel - vel_lin] - c through oracle.local
  gn_step        one Gauss-Newton iteration of a tail-only oracle chain that carries state Gaussians on some of its states
"""
import numpy as np

from oracle import oracle as O

# per-factor arrays of a problem description, by the key that holds the factor's (left) state; True: the factor touches state + 1 too
FACTOR_KEYS = {
    "gp_left": (["gp_dt"], True),
    "prior_idx": (["prior_pose", "prior_sig"], False),
    "vprior_idx": (["vprior", "vprior_sig"], False),
    "between_left": (["between_meas", "between_sig"], True),
    "range_left": (["range_lm", "range_z", "range_sigma", "range_dt", "range_tau"], True),
    "gps_left": (["gps_meas", "gps_sigma", "gps_dt", "gps_tau"], True),
    "att_left": (["att_nz", "att_bref", "att_sigma", "att_dt", "att_tau"], True),
}
PASS_KEYS = ("kind", "qc", "landmarks", "lprior_idx", "lprior", "lprior_sig")


def head_tail(p, k):
    """(head, tail) of problem p at state k: the head keeps states 0 .. k and every factor whose (left) state is < k; the tail keeps
    states k .. N - 1 and the other factors with their state indices lowered by k.  Landmarks and their priors go to the tail."""
    N = p["pose"].shape[0]
    head = dict(kind=p["kind"], qc=p["qc"], N=k + 1, pose=p["pose"][:k + 1].copy(), vel=p["vel"][:k + 1].copy())
    tail = dict(N=N - k, pose=p["pose"][k:].copy(), vel=p["vel"][k:].copy())
    for key in PASS_KEYS:
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


def sub_problem(p, lo, hi, new_from=None):
    """The states lo .. hi - 1 of problem p and the factors that touch only them -- with new_from, only those that also touch a state
    >= new_from (the factors a window gains when states new_from .. hi - 1 are appended).  State indices are lowered by lo."""
    out = dict(kind=p["kind"], qc=p["qc"], N=hi - lo, pose=p["pose"][lo:hi].copy(), vel=p["vel"][lo:hi].copy())
    for key, (others, two) in FACTOR_KEYS.items():
        if key not in p:
            continue
        idx = np.asarray(p[key])
        last = idx + (1 if two else 0)
        m = (idx >= lo) & (last < hi)
        if new_from is not None:
            m &= last >= new_from
        out[key] = (idx[m] - lo).astype(np.int32)
        for o in others:
            out[o] = np.asarray(p[o])[m]
    return out


def schur(D, Om, g, k, dtype=np.float64):
    """(Lambda, gamma, scale): D, Om, g the normal equations of a chain whose block k holds the head's share only (the head chain of
    head_tail); scale = max |diag D_k| before the subtraction."""
    D, Om, g = D.astype(dtype), Om.astype(dtype), g.astype(dtype)
    S, s = D[0].copy(), g[0].copy()
    for i in range(k):
        L = _chol(S)
        V = _fwd(L, Om[i].T)
        w = _fwd(L, s[:, None])[:, 0]
        S = D[i + 1] - V.T @ V
        s = g[i + 1] - V.T @ w
    return S, -s, float(np.abs(np.diag(D[k])).max())


def _chol(S):
    n = S.shape[0]
    L = np.zeros_like(S)
    for j in range(n):
        v = S[j, j] - (L[j, :j] * L[j, :j]).sum()
        assert v > 0
        L[j, j] = np.sqrt(v)
        for i in range(j + 1, n):
            L[i, j] = (S[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def _fwd(L, B):
    n = L.shape[0]
    X = np.zeros_like(B)
    for i in range(n):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def dense(D, Om):
    N, b = D.shape[0], D.shape[1]
    H = np.zeros((N * b, N * b))
    for i in range(N):
        H[i * b:(i + 1) * b, i * b:(i + 1) * b] = D[i]
        if i + 1 < N:
            H[(i + 1) * b:(i + 2) * b, i * b:(i + 1) * b] = Om[i]
            H[i * b:(i + 1) * b, (i + 1) * b:(i + 2) * b] = Om[i].T
    return H


def schur_dense(D, Om, g, k):
    """The same minimum through a dense inverse of the head's block (the check of `schur`)."""
    b = D.shape[1]
    H, gg = dense(D[:k + 1], Om[:k + 1]), g[:k + 1].reshape(-1)
    n = k * b
    Hhh, Hkh, Hkk = H[:n, :n], H[n:, :n], H[n:, n:]
    X = np.linalg.solve(Hhh, np.concatenate([Hkh.T, gg[:n, None]], 1))
    return Hkk - Hkh @ X[:, :b], -(gg[n:] - Hkh @ X[:, b])


def factor(Lam, gamma, scale):
    """A (b x b, zero rows behind the rank) and c with A^T A = sym(Lam), A^T c = -gamma: Cholesky with diagonal pivoting, pivots at
    or below b eps scale end it."""
    b = Lam.shape[0]
    W = 0.5 * (Lam + Lam.T)
    thr = b * np.finfo(float).eps * scale
    perm = list(range(b))
    L = np.zeros((b, b))
    rank = 0
    for j in range(b):
        q = j + int(np.argmax(np.diag(W)[j:]))
        if q != j:
            perm[j], perm[q] = perm[q], perm[j]
            W[[j, q], :] = W[[q, j], :]
            W[:, [j, q]] = W[:, [q, j]]
            L[[j, q], :j] = L[[q, j], :j]
        if not W[j, j] > thr:
            break
        L[j, j] = np.sqrt(W[j, j])
        L[j + 1:, j] = W[j + 1:, j] / L[j, j]
        W[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
        rank = j + 1
    A, c = np.zeros((b, b)), np.zeros(b)
    rhs = -np.asarray(gamma)
    for i in range(rank):
        for m in range(i, b):
            A[i, perm[m]] = L[m, i]
        c[i] = (rhs[perm[i]] - L[i, :i] @ c[:i]) / L[i, i]
    return A, c


def xi_of(kind, chart, pose_lin, vel_lin, pose, vel):
    return np.concatenate([O.local(kind, pose_lin, pose, chart), np.asarray(vel) - np.asarray(vel_lin)])


def residual(kind, chart, pose_lin, vel_lin, A, c, pose, vel):
    return A @ xi_of(kind, chart, pose_lin, vel_lin, pose, vel) - c


def gn_step(orc, kind, chart, gaussians):
    """One Gauss-Newton iteration of the oracle chain `orc` (the tail's factors) with state Gaussians (idx, pose_lin, vel_lin, A, c):
    the oracle's normal equations, A^T A on the block and A^T (c - A xi) on the gradient (the oracle's g is -J^T e), the oracle's
    block-tridiagonal solve and retraction.  Returns (pose, vel) and leaves them in orc."""
    pose, vel = orc.get_states()
    D, Om, g = orc.normal_equations()[:3]
    d = O.TANGENT_DIM[kind]
    for idx, pl, vl, A, c in gaussians:
        xi = xi_of(kind, chart, pl, vl, pose[idx], vel[idx])
        D[idx] += A.T @ A
        g[idx] += A.T @ (c - A @ xi)
    x = O.block_tridiag_solve(D, Om, g)
    pose = np.stack([O.retract(kind, pose[i], x[i, :d], chart) for i in range(pose.shape[0])])
    vel = vel + x[:, d:]
    orc.set_states(pose, vel)
    return pose, vel
