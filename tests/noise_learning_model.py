"""numpy model of gpslam_hip_meas_noise_statistic / gpslam_hip_meas_predicted_covariances and of the host arithmetic behind them
(gpslam_amd/csrc/meas_noise.hip, include/gpslam_hip_noise.h): B, Bw, n and the per-factor P_m = J_m Sigma_m J_m^T from a dense
Sigma = inv(H) -- or from the four outputs of get_marginals(cross=True) -- and the unwhitened measurement linearisation (e, J as
linearize_meas returns them), the derivative G of the log-evidence in W = C^-1 at fixed states, the EM update and the stationary
scales; a linear-Gaussian problem y = C x + nu with its textbook likelihood; and what a description of tests/fixed_lag_mix_model.py
says about one measurement kind (indices, landmarks, base whitening)."""
import numpy as np


def sigma_of(Sigma, N, b, ld, i, l, two):
    """Sigma_m of a factor on state i (and i + 1 if two) and landmark l (None: none): from the dense covariance in the order
    [states | landmarks], or from (S, S_next, S_x_lm, S_lm) as get_marginals(cross=True) returns them (S_x_lm: N x b x nl)"""
    ns = 2 if two else 1
    if isinstance(Sigma, tuple):
        Sd, Sn, Sxl, Slm = Sigma
        top = np.block([[Sd[i], Sn[i]], [Sn[i].T, Sd[i + 1]]]) if two else Sd[i]
        if l is None:
            return top
        c = slice(l * ld, (l + 1) * ld)
        X = np.vstack([Sxl[i + s][:, c] for s in range(ns)])
        return np.block([[top, X], [X.T, Slm[c, c]]])
    rows = np.arange(i * b, (i + ns) * b)
    if l is not None:
        rows = np.concatenate([rows, N * b + l * ld + np.arange(ld)])
    return Sigma[np.ix_(rows, rows)]


def statistic(Sigma, e, J, idx, lm, R, use=None, N=None, ld=0, two=True):
    """(B, Bw, n, P, scales) over the factors with use[f] (all by default): e (count x r), J (count x r x (2 b + 3)) = [H1 H2 | H3 H4
    | H5 padded to 3], idx the left (or only) state, lm the landmark per factor or None, R (count x r x r) the base whitening.  P
    holds every factor's J Sigma_m J^T, used or not.  scales: what an entrywise error bound is made of -- cov = sum |J| (dg dg^T)
    |J|^T with dg = sqrt(diag Sigma_m) (an error of tol in correlation units on Sigma_m moves B by at most tol * cov), err =
    sum |e| |e|^T, cov_w / err_w the same with R J and R e, cov_P the per-factor |J| (dg dg^T) |J|^T."""
    e, J, R = np.asarray(e, dtype=float), np.asarray(J, dtype=float), np.asarray(R, dtype=float)
    M, r = e.shape
    b = (J.shape[2] - 3) // 2
    if N is None:
        N = Sigma[0].shape[0] if isinstance(Sigma, tuple) else Sigma.shape[0] // b
    B, Bw = np.zeros((r, r)), np.zeros((r, r))
    sc = {k: np.zeros((r, r)) for k in ("cov", "err", "cov_w", "err_w")}
    P, covP = np.zeros((M, r, r)), np.zeros((M, r, r))
    n = 0
    for f in range(M):
        i = int(idx[f])
        l = None if lm is None else int(lm[f])
        Sm = sigma_of(Sigma, N, b, ld, i, l, two)
        cols = list(range(2 * b if two else b)) + ([] if l is None else list(range(2 * b, 2 * b + ld)))
        Jm = J[f][:, cols]
        dg = np.sqrt(np.maximum(np.diag(Sm), 0.0))
        P[f] = Jm @ Sm @ Jm.T
        covP[f] = np.abs(Jm) @ np.outer(dg, dg) @ np.abs(Jm).T
        if use is not None and not use[f]:
            continue
        U = np.outer(e[f], e[f]) + P[f]
        B += U
        Bw += R[f] @ U @ R[f].T
        RJ, Re = R[f] @ Jm, R[f] @ e[f]
        sc["cov"] += covP[f]
        sc["err"] += np.outer(np.abs(e[f]), np.abs(e[f]))
        sc["cov_w"] += np.abs(RJ) @ np.outer(dg, dg) @ np.abs(RJ).T
        sc["err_w"] += np.outer(np.abs(Re), np.abs(Re))
        n += 1
    sc["cov_P"] = covP
    return B, Bw, n, P, sc


def gradient(C, B, n):
    """G with dF = tr(G dW), W = C^-1: (n C - B) / 2"""
    return 0.5 * (n * np.asarray(C) - np.asarray(B))


def em_update(B, n):
    return 0.5 * (B + B.T) / n


def em_scale(Bw, n):
    """(theta+ / theta, the per-row ratios)"""
    r = Bw.shape[0]
    return float(np.trace(Bw)) / (n * r), np.diag(Bw) / n


def sqrt_information(cov):
    """upper R with R^T R = cov^-1, as gpslam_hip_set_meas_covariance stores it"""
    return np.linalg.cholesky(np.linalg.inv(cov)).T


# ---------------------------------------------------------------- a description's measurement kinds (tests/fixed_lag_mix_model.py)
def kind_of(p, pre):
    """(MEAS_* kind, idx, lm or None, two, rows, ld, R) of the factors of one prefix of a plain description"""
    import fixed_lag_mix_model as FM
    mk, key, two, rows, haslm, _ = FM.MEAS[pre]
    idx = np.asarray(p[key])
    M = len(idx)
    sig = np.asarray(p[pre + "_sigma"], dtype=float).reshape(M, rows)
    R = np.stack([np.diag(1.0 / s) for s in sig]) if M else np.zeros((0, rows, rows))
    if pre + "_cov" in p:
        cov = np.asarray(p[pre + "_cov"])
        for f in np.nonzero(np.isfinite(cov).all(axis=(1, 2)))[0]:
            R[f] = sqrt_information(cov[f])
    return mk, idx, (np.asarray(p[pre + "_lm"]) if haslm else None), two, rows, (int(p.get("ld", 0)) if haslm else 0), R


def kinds(p):
    import fixed_lag_mix_model as FM
    return [pre for pre in FM.MEAS if FM.MEAS[pre][1] in p and len(p[FM.MEAS[pre][1]])]


def bounds(tol, ref, sc, rel=1e-11):
    """the entrywise bounds of (B, Bw, P): tol * cov + rel * (err + |ref|); P per factor, without an error term"""
    B, Bw, _, P = ref[:4]
    return (tol * sc["cov"] + rel * (sc["err"] + np.abs(B)), tol * sc["cov_w"] + rel * (sc["err_w"] + np.abs(Bw)),
            tol * sc["cov_P"] + rel * np.abs(P))


# ---------------------------------------------------------------- the linear-Gaussian problem y = C x + nu
def linear_problem(N=12, b=4, r=2, seed=0, shapes=False):
    """x = (x_0 .. x_N-1) ~ N(m, K), K a dense SPD matrix; measurement f looks at the states idx[f], idx[f] + 1 through C_f
    (r x 2 b) and adds nu_f ~ N(0, theta_true C0_f).  shapes: every factor has its own C0_f (the scale family), else one C0."""
    rng = np.random.default_rng(seed)
    nx = N * b
    G = rng.standard_normal((nx, nx)) / np.sqrt(nx)
    K = G @ G.T + 0.3 * np.eye(nx)
    m = rng.standard_normal(nx)
    idx = np.concatenate([np.arange(N - 1), rng.integers(0, N - 1, 3 * N)]).astype(np.int32)
    M = len(idx)
    Cf = rng.standard_normal((M, r, 2 * b))
    base = np.array([[1.0, 0.3], [0.3, 0.6]])[:r, :r]
    C0 = np.stack([base * (1.0 + 0.5 * rng.random()) + np.diag(0.3 * rng.random(r)) for _ in range(M)]) if shapes else np.tile(base, (M, 1, 1))
    theta_true = 0.7
    x = m + np.linalg.cholesky(K) @ rng.standard_normal(nx)
    y = np.stack([Cf[f] @ x[idx[f] * b:(idx[f] + 2) * b] + np.linalg.cholesky(theta_true * C0[f]) @ rng.standard_normal(r) for f in range(M)])
    return dict(N=N, b=b, r=r, K=K, m=m, idx=idx, C=Cf, C0=C0, y=y, theta_true=theta_true)


def _stacked(pr):
    N, b, r = pr["N"], pr["b"], pr["r"]
    M = len(pr["idx"])
    Call = np.zeros((M * r, N * b))
    for f in range(M):
        Call[f * r:(f + 1) * r, pr["idx"][f] * b:(pr["idx"][f] + 2) * b] = pr["C"][f]
    return Call


def textbook(pr, cov):
    """(log N(y; C m, C K C^T + blockdiag(cov_f)), the magnitude its rounding scales with): no J, no H, no posterior"""
    r = pr["r"]
    M = len(pr["idx"])
    Call = _stacked(pr)
    S = Call @ pr["K"] @ Call.T
    for f in range(M):
        S[f * r:(f + 1) * r, f * r:(f + 1) * r] += cov[f]
    L = np.linalg.cholesky(S)
    z = np.linalg.solve(L, pr["y"].reshape(-1) - Call @ pr["m"])
    ld = np.log(np.diag(L))
    return -0.5 * float(z @ z) - float(ld.sum()) - 0.5 * M * r * np.log(2.0 * np.pi), 0.5 * float(z @ z) + float(np.abs(ld).sum())


def linear_statistic(pr, cov, use=None):
    """(B, Bw, n, P, scales) of the linear problem at its posterior mean under the factor covariances cov (count x r x r)"""
    N, b, r = pr["N"], pr["b"], pr["r"]
    M = len(pr["idx"])
    Call = _stacked(pr)
    Wall = np.zeros((M * r, M * r))
    for f in range(M):
        Wall[f * r:(f + 1) * r, f * r:(f + 1) * r] = np.linalg.inv(cov[f])
    Ki = np.linalg.inv(pr["K"])
    H = Ki + Call.T @ Wall @ Call
    Sig = np.linalg.inv(H)
    xh = Sig @ (Ki @ pr["m"] + Call.T @ Wall @ pr["y"].reshape(-1))
    e = (Call @ xh).reshape(M, r) - pr["y"]
    J = np.zeros((M, r, 2 * b + 3))
    J[:, :, :2 * b] = pr["C"]
    R = np.stack([sqrt_information(c) for c in cov])
    return statistic(Sig, e, J, pr["idx"], None, R, use, N=N, two=True)


# ---------------------------------------------------------------- the learning problem of tests/test_gpu_noise_learning.py
LEARN_SEED = 4
C_TRUE = np.array([[0.04, 0.012, -0.008], [0.012, 0.025, 0.006], [-0.008, 0.006, 0.0625]])


def learn_problem():
    """40 SE(3) states with odometry, 4 interpolated GPS factors per interval whose noise is drawn at C_TRUE around the optimum of the
    graph without them"""
    from gpslam_amd import synthetic as S
    from oracle import oracle as O
    p = dict(S.pose3_gps_chain(40, per_interval=4, keep_odometry=True))
    M = len(p["gps_left"])
    q = dict(p, gps_meas=np.zeros((M, 3)))
    orc = S.apply({k: v for k, v in q.items() if not k.startswith("gps_")}, O.Chain(O.POSE3))
    for _ in range(4):
        orc.iterate_gn()
    truth = orc.get_states()
    orc = S.apply(dict(q, pose=truth[0], vel=truth[1]), O.Chain(O.POSE3))
    pred, _ = orc.linearize_meas(3, M)
    rng = np.random.default_rng(LEARN_SEED)
    p["gps_meas"] = pred + rng.standard_normal((M, 3)) @ np.linalg.cholesky(C_TRUE).T
    return p


def model_learn(p, mode, cov_start, steps, params, with_qc=None):
    """evidence.learn_meas_noise's loop on the oracle with the numpy model in the place of the device's statistic: the list of what is
    learned, one entry per model evaluated"""
    from gpslam_amd import synthetic as S
    from oracle import oracle as O
    import marginals_model as MM
    import qc_learning_model as QM
    M, N = len(p["gps_left"]), p["N"]
    orc = S.apply(p, O.Chain(O.POSE3))
    cov0 = np.tile(cov_start, (M, 1, 1))
    theta = 1.0 if mode == "scale" else (np.ones(3) if mode == "rows" else np.array(cov_start, dtype=float))
    Qc = None if with_qc is None else np.array(with_qc[0], dtype=float)
    out = []
    for _ in range(steps):
        cov = theta * cov0 if mode == "scale" else (cov0 * np.diag(theta) if mode == "rows" else np.tile(theta, (M, 1, 1)))
        orc.set_meas_covariance(3, cov)
        if Qc is not None:
            orc.set_qc(Qc)
        orc.set_states(p["pose"], p["vel"])
        orc.compile()
        orc.optimize(params)
        D, O_, _, _, _, _ = orc.normal_equations()
        Sig = np.linalg.inv(MM.dense(D, O_))
        e, J = orc.linearize_meas(3, M)
        R = np.stack([sqrt_information(c) for c in cov])
        B, Bw, n, _, _ = statistic(Sig, e, J, p["gps_left"], None, R, N=N, two=True)
        out.append((np.copy(theta), None if Qc is None else Qc.copy()))
        theta = theta * em_scale(Bw, n)[0] if mode == "scale" else (theta * em_scale(Bw, n)[1] if mode == "rows" else em_update(B, n))
        if Qc is not None:
            eg, Hq = orc.linearize_gp()
            A, n_f, _, _ = QM.statistic(Sig, eg, Hq, p["gp_left"], p["gp_dt"], 12)
            Qc = QM.em_scale(with_qc[0], A, n_f) * with_qc[0] if with_qc[1] else QM.em_update(A, n_f)
    return out


def tight(params):
    """a fixed number of Gauss-Newton iterations on both sides: the stopping rules of the two optimisers never decide"""
    params.max_iterations = 6
    params.relative_error_tol = params.absolute_error_tol = params.error_tol = params.delta_tol = 0.0
    return params
