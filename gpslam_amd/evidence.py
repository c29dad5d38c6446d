"""Choosing Qc by the Laplace log-evidence (include/gpslam_hip_evidence.h): a sweep over scales of a given Qc0, Qc learned by
expectation-maximisation (learn_qc), and the measurement noise of one kind learned the same way (learn_meas_noise).

Standard GP-regression practice picks the hyperparameter that maximises the marginal likelihood of the data; for this nonlinear
least-squares problem that is log Z = -cost(x^) + sum_f log|det R_f| - 1/2 log det H - ((m - n) / 2) log 2 pi at the optimum x^
(ChainSolver.log_evidence).  The GP priors must carry the handle's Qc (add_gp_priors, not add_gp_priors_qc) for set_qc to reach them.
"""
import numpy as np

from .chain import GpslamHipError, noise_em_scale, noise_em_update, qc_em_scale, qc_em_update


def qc_scale_sweep(solver, Qc0, scales, pose0, vel0, landmarks0=None, params=None):
    """For each theta in scales: set_qc(theta * Qc0), the states (and landmarks) back to the same start, compile, optimize(params),
    log_evidence.  Returns (out5, iterations): out5[k] = (log Z, cost, log det H, lognorm, m - n) at theta = scales[k], and the
    optimiser's iteration count there.  The solver is left at the last scale's optimum."""
    Qc0 = np.asarray(Qc0, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64).reshape(-1)
    out5 = np.zeros((len(scales), 5))
    iterations = np.zeros(len(scales), dtype=np.int64)
    for k, theta in enumerate(scales):
        solver.set_qc(theta * Qc0)
        solver.set_states(pose0, vel0)
        if landmarks0 is not None:
            solver.set_landmarks(landmarks0)
        solver.compile()
        _, st = solver.optimize(params)
        iterations[k] = st.iterations
        out5[k] = solver.log_evidence()
    return out5, iterations


def learn_qc(solver, Qc0, pose0, vel0, landmarks0=None, params=None, steps=10, rtol=1e-6, scale_only=False):
    """Learn Qc by expectation-maximisation (include/gpslam_hip_qc.h): instead of a grid, each step evaluates ONE Qc -- set_qc, the
    states (and landmarks) back to the same start, compile, optimize(params), marginals, qc_statistic -- and moves to the stationary
    point of the log-evidence at those states, Qc+ = A / (2 n_f); scale_only=True keeps the shape of Qc0 and learns theta alone,
    Qc+ = theta+ Qc0 with theta+ = tr(Qc0^-1 A) / (2 n_f d).  Stops after `steps` steps or once |Qc+ - Qc|_F <= rtol |Qc|_F.
    Returns the list of (Qc, log Z, iterations), one entry per Qc evaluated; log Z is None where log_evidence refuses the graph (robust
    losses, the segmented landmark path, ...).  The solver is left at the optimum of the last entry's Qc, which is what it holds;
    its marginals are stale (log_evidence rewrites the solver's buffers)."""
    Qc0 = np.array(Qc0, dtype=np.float64)
    Qc = Qc0.copy()
    out = []
    for _ in range(int(steps)):
        solver.set_qc(Qc)
        solver.set_states(pose0, vel0)
        if landmarks0 is not None:
            solver.set_landmarks(landmarks0)
        solver.compile()
        _, st = solver.optimize(params)
        solver.marginals()
        A, n_f = solver.qc_statistic()
        try:
            logz = solver.log_evidence()[0]
        except GpslamHipError as err:
            if "(-5)" not in str(err):      # GPSLAM_E_UNSUPPORTED; anything else is an error here as well
                raise
            logz = None
        out.append((Qc.copy(), logz, int(st.iterations)))
        if n_f == 0:
            break               # no prior carries the shared Qc: there is nothing to learn
        nxt = qc_em_scale(Qc0, A, n_f) * Qc0 if scale_only else qc_em_update(A, n_f)
        done = np.linalg.norm(nxt - Qc) <= rtol * np.linalg.norm(Qc)
        Qc = nxt
        if done:
            break
    return out


def _log_evidence_or_none(solver):
    try:
        return solver.log_evidence()[0]
    except GpslamHipError as err:
        if "(-5)" not in str(err):      # GPSLAM_E_UNSUPPORTED; anything else is an error here as well
            raise
        return None


def learn_meas_noise(solver, kind, pose0, vel0, landmarks0=None, params=None, steps=10, rtol=1e-6, mode="scale", use=None, with_qc=None,
                     cov0=None):
    """Learn the measurement noise of one MEAS_* kind by expectation-maximisation (include/gpslam_hip_noise.h).  cov0: the covariances
    the kind's factors start from, (count, r, r) or one (r, r) for all -- the handle has no getter for them, so they are an argument;
    `use` (one entry per factor, None: all) names the factors that are learned, the others keep cov0.  Each step evaluates ONE noise
    model -- set_meas_covariance on every factor of the kind, the states (and landmarks) back to the same start, compile,
    optimize(params), marginals, meas_noise_statistic -- and moves to the stationary point of the log-evidence at those states:
      mode="scale":  C_m = theta C_m^0, theta+ = theta tr(Bw) / (n r)            (every factor keeps its shape);
      mode="rows":   C_m = diag(theta) C_m^0 for diagonal C_m^0, theta_q+ = theta_q Bw[q, q] / n;
      mode="shared": the used factors share one C, C+ = B / n.
    with_qc=(Qc0, scale_only): qc_statistic is taken from the same marginals and Qc moves with learn_qc's update in the same loop.
    Stops after `steps` steps or once the relative change of what is learned is at most rtol.  Returns the list of
    (theta | C, log Z, iterations), one entry per model evaluated ((theta | C, Qc) in the first place with with_qc); log Z is None where
    log_evidence refuses the graph.  The solver is left at the optimum of the last entry's model, which is what it holds; its
    marginals are stale (log_evidence rewrites the solver's buffers)."""
    if mode not in ("scale", "rows", "shared"):
        raise GpslamHipError("learn_meas_noise: mode must be 'scale', 'rows' or 'shared'")
    if cov0 is None:
        raise GpslamHipError("learn_meas_noise: cov0 (the covariances the factors start from) is needed")
    kind = int(kind)
    r = solver.MEAS_ROWS[kind]
    count = solver.meas_count(kind)
    cov0 = np.array(np.broadcast_to(np.asarray(cov0, dtype=np.float64).reshape(-1, r, r), (count, r, r)))
    used = np.ones(count, dtype=bool) if use is None else np.asarray(use).reshape(-1) != 0
    if len(used) != count:
        raise GpslamHipError("learn_meas_noise: `use` has %d entries, the kind has %d factors" % (len(used), count))
    if mode == "rows" and np.any(cov0[used] != cov0[used] * np.eye(r)):
        raise GpslamHipError("learn_meas_noise: mode='rows' needs diagonal covariances")
    theta = 1.0 if mode == "scale" else (np.ones(r) if mode == "rows" else cov0[used][0].copy() if used.any() else np.eye(r))
    Qc0 = Qc = None
    if with_qc is not None:
        Qc0 = np.array(with_qc[0], dtype=np.float64)
        Qc = Qc0.copy()
    out = []
    for _ in range(int(steps)):
        cov = cov0.copy()
        if mode == "scale":
            cov[used] = theta * cov0[used]
        elif mode == "rows":
            cov[used] = cov0[used] * np.diag(theta)
        else:
            cov[used] = theta
        solver.set_meas_covariance(kind, cov)
        if Qc is not None:
            solver.set_qc(Qc)
        solver.set_states(pose0, vel0)
        if landmarks0 is not None:
            solver.set_landmarks(landmarks0)
        solver.compile()
        _, st = solver.optimize(params)
        solver.marginals()
        B, Bw, n = solver.meas_noise_statistic(kind, None if use is None else used)
        if Qc is not None:
            A, n_f = solver.qc_statistic()
        logz = _log_evidence_or_none(solver)
        here = np.copy(theta) if mode != "scale" else float(theta)
        out.append(((here, Qc.copy()) if Qc is not None else here, logz, int(st.iterations)))
        if n == 0:
            break               # no factor is used: there is nothing to learn
        if mode == "scale":
            nxt = theta * noise_em_scale(Bw, n)[0]
        elif mode == "rows":
            nxt = theta * noise_em_scale(Bw, n)[1]
        else:
            nxt = noise_em_update(B, n)
        done = np.linalg.norm(np.asarray(nxt) - np.asarray(theta)) <= rtol * np.linalg.norm(np.asarray(theta))
        theta = nxt
        if Qc is not None and n_f > 0:
            qn = qc_em_scale(Qc0, A, n_f) * Qc0 if with_qc[1] else qc_em_update(A, n_f)
            done = done and np.linalg.norm(qn - Qc) <= rtol * np.linalg.norm(Qc)
            Qc = qn
        if done:
            break
    return out
