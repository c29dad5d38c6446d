"""Choosing Qc by the Laplace log-evidence (include/gpslam_hip_evidence.h): a sweep over scales of a given Qc0.

Standard GP-regression practice picks the hyperparameter that maximises the marginal likelihood of the data; for this nonlinear
least-squares problem that is log Z = -cost(x^) + sum_f log|det R_f| - 1/2 log det H - ((m - n) / 2) log 2 pi at the optimum x^
(ChainSolver.log_evidence).  The GP priors must carry the handle's Qc (add_gp_priors, not add_gp_priors_qc) for set_qc to reach them.
"""
import numpy as np


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
