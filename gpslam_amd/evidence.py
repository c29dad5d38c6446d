"""Choosing Qc by the Laplace log-evidence (include/gpslam_hip_evidence.h): a sweep over scales of a given Qc0.

Standard GP-regression practice picks the hyperparameter that maximises the marginal likelihood of the data; for this nonlinear
least-squares problem that is log Z = -cost(x^) + sum_f log|det R_f| - 1/2 log det H - ((m - n) / 2) log 2 pi at the optimum x^
(ChainSolver.log_evidence).  The GP priors must carry the handle's Qc (add_gp_priors, not add_gp_priors_qc) for set_qc to reach them.
"""
import numpy as np

from .chain import GpslamHipError, qc_em_scale, qc_em_update


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
