"""numpy model of gpslam_hip_qc_statistic and of the host arithmetic behind it (gpslam_amd/csrc/qc_learn.hip, include/gpslam_hip_qc.h):
the statistic A from a dense Sigma = inv(H) and the unwhitened GP-prior linearisation (e, H1..H4 as linearize_gp returns them), the
derivative G of the log-evidence in W = Qc^-1 at fixed states, the EM update and the stationary scale."""
import numpy as np

import evidence_model as EM


def time_whiten(e, Hq, dt):
    """[(e~_1, J~_1), (e~_2, J~_2)] of one prior: e (2d), Hq (4, 2d, d) -- block q the columns of [x_i, v_i, x_i+1, v_i+1], rows
    [top d; bottom d] -- whitened by K = [[sa, sb], [0, sc]], K^T K = [[12 / dt^3, -6 / dt^2], [-6 / dt^2, 4 / dt]]"""
    d = Hq.shape[2]
    J = np.hstack([Hq[q] for q in range(4)])          # 2d x 4d
    sa = np.sqrt(12.0 / dt ** 3)
    sb = (-6.0 / dt ** 2) / sa
    sc = 1.0 / np.sqrt(dt)
    return [(sa * e[:d] + sb * e[d:], sa * J[:d] + sb * J[d:]), (sc * e[d:], sc * J[d:])]


def statistic(Sigma, e, Hq, left, dts, b, use=None):
    """(A, n_f, cov_scale, err_scale): A = sum_i sum_k (e~_k e~_k^T + J~_k Sigma_J J~_k^T) over the priors with use[f] (all of them
    by default), Sigma the dense covariance in the states' order (landmark columns behind them are ignored) or the pair
    (S, S_next) of get_marginals.  The two scales are what
    an entrywise error bound of A is made of: cov_scale = sum |J~_k| (dg dg^T) |J~_k|^T with dg = sqrt(diag Sigma_J) -- an error of
    tol in correlation units on S / S_next moves A by at most tol * cov_scale -- and err_scale = sum |e~_k| |e~_k|^T."""
    d = b // 2
    A, cov_scale, err_scale = np.zeros((d, d)), np.zeros((d, d)), np.zeros((d, d))
    n_f = 0
    for f in range(len(left)):
        if use is not None and not use[f]:
            continue
        i = int(left[f])
        if isinstance(Sigma, tuple):        # (S, S_next) as get_marginals returns them
            Sd, Sn = Sigma
            SJ = np.block([[Sd[i], Sn[i]], [Sn[i].T, Sd[i + 1]]])
        else:
            r = slice(i * b, (i + 2) * b)
            SJ = Sigma[r, r]
        dg = np.sqrt(np.maximum(np.diag(SJ), 0.0))
        for et, Jt in time_whiten(e[f], Hq[f], float(dts[f])):
            A += np.outer(et, et) + Jt @ SJ @ Jt.T
            cov_scale += np.abs(Jt) @ np.outer(dg, dg) @ np.abs(Jt).T
            err_scale += np.outer(np.abs(et), np.abs(et))
        n_f += 1
    return A, n_f, cov_scale, err_scale


def gradient(Qc, A, n_f):
    """G with dF = tr(G dW), W = Qc^-1: n_f Qc - A / 2"""
    return n_f * np.asarray(Qc) - 0.5 * np.asarray(A)


def em_update(A, n_f):
    return 0.5 * (A + A.T) / (2.0 * n_f)


def em_scale(Qc0, A, n_f):
    return float(np.trace(np.linalg.solve(Qc0, A))) / (2.0 * n_f * Qc0.shape[0])


def textbook(pr, Qc):
    """the textbook log-evidence of the linear problem at Qc: no J and no H"""
    return EM.gp_marginal_loglik(pr["m0"], pr["P0"], pr["dts"], Qc, pr["meas_idx"], pr["y"], pr["sig"])


def linear_chain(pr, Qc):
    """The oracle's chain for EM.linear_gp_problem at Qc, at its optimum (every factor is linear: two Gauss-Newton steps)"""
    from oracle import oracle as O
    N, d = pr["N"], pr["d"]
    orc = O.Chain(O.LINEAR3 if d == 3 else O.LINEAR2)
    orc.set_qc(Qc)
    orc.set_states(np.zeros((N, d)), np.zeros((N, d)))
    orc.add_gp_priors(np.arange(N - 1, dtype=np.int32), pr["dts"])
    orc.add_pose_priors(np.array([0], dtype=np.int32), pr["m0"][None, :d], pr["sp"][None])
    orc.add_vel_priors(np.array([0], dtype=np.int32), pr["m0"][None, d:], pr["sv"][None])
    orc.add_pose_priors(pr["meas_idx"], pr["y"], pr["sig"])
    orc.compile()
    for _ in range(2):
        rc, _ = orc.iterate_gn()
        assert rc == 0
    return orc


def linear_statistic(pr, Qc, scales=False):
    """(A, n_f, H) of the linear problem at its optimum for Qc, from a dense inverse of the oracle's H and its linearize_gp();
    scales: (A, n_f, H, cov_scale, err_scale)"""
    import marginals_model as MM
    orc = linear_chain(pr, Qc)
    D, O_, _, _, _, _ = orc.normal_equations()
    H = MM.dense(D, O_)
    e, Hq = orc.linearize_gp()
    A, n_f, cov_scale, err_scale = statistic(np.linalg.inv(H), e, Hq, np.arange(pr["N"] - 1), pr["dts"], 2 * pr["d"])
    return (A, n_f, H, cov_scale, err_scale) if scales else (A, n_f, H)


def em_fixed_point(pr, Qc, steps, rtol=0.0, scale_of=None):
    """EM from Qc: the list of Qc visited (the start included).  scale_of: learn theta of theta * scale_of alone"""
    out = [np.array(Qc, dtype=float)]
    for _ in range(steps):
        A, n_f, _ = linear_statistic(pr, out[-1])
        nxt = em_scale(scale_of, A, n_f) * scale_of if scale_of is not None else em_update(A, n_f)
        done = np.linalg.norm(nxt - out[-1]) <= rtol * np.linalg.norm(out[-1])
        out.append(nxt)
        if done:
            break
    return out
