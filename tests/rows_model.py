"""numpy model of the row tables gpslam_hip_get_rows returns (include/gpslam_hip.h): where every factor's whitened rows sit, and
the normal equations those rows assemble to.

FactorLists has the call surface of gpslam_amd.ChainSolver / oracle.Chain and only records: a recipe written for a solver feeds it
unchanged, and the recording is replayed into as many handles as a test needs (optionally edited on the way, e.g. translated).
row_map() places the rows the way the header documents it:

    full-width rows grouped by left state; inside a state GP priors, velocity priors, then the measurement kinds in GPSLAM_MEAS_*
    order, each in the order added; then the velocity-free rows (pose priors, between factors), again grouped by left state.

assemble() forms D, O, g, B, HLL, gL from (rowLR, rowE, rowM, rowLm) and that map in the conventions of
gpslam_hip_normal_equations / oracle.Chain.normal_equations: O[i] = H[i+1, i], g = -J^T e."""
import numpy as np

EPS = np.finfo(float).eps
MEAS_ROWS = {0: 1, 1: 1, 2: 2, 3: 3, 4: 3, 5: 2, 6: 2, 7: 3}       # rows per factor of each GPSLAM_MEAS_* kind
MEAS_CALL = {"add_interp_range": 0, "add_range": 1, "add_interp_attitude": 2, "add_interp_gps": 3, "add_odometry2d": 4,
             "add_bearing_range": 5, "add_interp_projection": 6, "add_ahrs": 7}
MEAS_NAMES = {0: "interp-range", 1: "range", 2: "interp-attitude", 3: "interp-gps", 4: "odometry2d", 5: "bearing-range",
              6: "interp-projection", 7: "ahrs"}


class RowMap:
    """left[r]: left state of row r of get_rows(); row0[set][f]: first row of factor f of a set ('gp', 'vpri', 'pri', 'btw' or a
    GPSLAM_MEAS_* number), rows[set]: its row count; M / Mc: rows of the full-width / velocity-free part."""

    def __init__(self, left, row0, rows, M, Mc):
        self.left, self.row0, self.rows, self.M, self.Mc = left, row0, rows, M, Mc

    def rows_of(self, key, f=None):
        """row indices of one factor, or of every factor of the set (factor-major)"""
        r0 = self.row0[key] if f is None else self.row0[key][f:f + 1]
        return (np.asarray(r0)[:, None] + np.arange(self.rows[key])[None, :]).ravel()


def row_map(N, d, gp_left=(), vpri_idx=(), pri_idx=(), btw_left=(), meas=None):
    """meas: {GPSLAM_MEAS_* kind: left states in the order added}"""
    b = 2 * d
    meas = meas or {}
    full = [("gp", np.asarray(gp_left, dtype=int), b), ("vpri", np.asarray(vpri_idx, dtype=int), d)]
    full += [(k, np.asarray(meas[k], dtype=int), MEAS_ROWS[k]) for k in sorted(meas)]
    compact = [("pri", np.asarray(pri_idx, dtype=int), d), ("btw", np.asarray(btw_left, dtype=int), d)]
    row0, rows, lefts, base = {}, {}, [], 0
    for table in (full, compact):
        count = np.zeros(N, dtype=int)
        for _, idx, n in table:
            np.add.at(count, idx, n)
        ptr = np.concatenate([[0], np.cumsum(count)])
        cursor = ptr[:-1].copy()
        for key, idx, n in table:
            r0 = np.zeros(len(idx), dtype=int)
            for f, s in enumerate(idx):
                r0[f] = base + cursor[s]
                cursor[s] += n
            row0[key], rows[key] = r0, n
        lefts.append(np.repeat(np.arange(N), count))
        base += ptr[-1]
    return RowMap(np.concatenate(lefts), row0, rows, len(lefts[0]), len(lefts[1]))


def assemble(N, b, left, rowLR, rowE, rowM=None, rowLm=None, L=0, ld=0, lprior=None):
    """D (N, b, b), O (N, b, b), g (N, b), B (N, b, L ld), HLL, gL of the rows.  lprior = (idx, sigmas[, residual]): the landmark
    priors, which have no rows in the tables, add 1 / sigma^2 to HLL's diagonal (and -residual / sigma^2 to gL)."""
    D, O, g = np.zeros((N, b, b)), np.zeros((N, b, b)), np.zeros((N, b))
    nl = L * ld
    B = np.zeros((N, b, nl)) if nl else None
    HLL = np.zeros((nl, nl)) if nl else None
    gL = np.zeros(nl) if nl else None
    assert len(left) == len(rowLR) == len(rowE)
    for r, s in enumerate(left):
        JL, JR, e = rowLR[r, :b], rowLR[r, b:], rowE[r]
        D[s] += np.outer(JL, JL)
        g[s] -= JL * e
        if s + 1 < N:
            D[s + 1] += np.outer(JR, JR)
            O[s] += np.outer(JR, JL)
            g[s + 1] -= JR * e
        else:
            assert not JR.any(), "row %d of the last state has a right half" % r
        if nl and rowLm[r] >= 0:
            c = slice(rowLm[r] * ld, rowLm[r] * ld + ld)
            Jm = rowM[r]
            B[s][:, c] += np.outer(JL, Jm)
            if s + 1 < N:
                B[s + 1][:, c] += np.outer(JR, Jm)
            HLL[c, c] += np.outer(Jm, Jm)
            gL[c] -= Jm * e
    if nl and lprior is not None:
        idx, sig = np.asarray(lprior[0], dtype=int), np.asarray(lprior[1], dtype=float).reshape(-1, ld)
        for k, l in enumerate(idx):
            for q in range(ld):
                HLL[l * ld + q, l * ld + q] += 1.0 / sig[k, q] ** 2
                if len(lprior) > 2:
                    gL[l * ld + q] -= np.asarray(lprior[2]).reshape(-1, ld)[k, q] / sig[k, q] ** 2
    return D, O, g, B, HLL, gL


def dense(D, O, B=None, HLL=None):
    N, b = D.shape[0], D.shape[1]
    A = np.zeros((N * b, N * b))
    for i in range(N):
        A[i * b:(i + 1) * b, i * b:(i + 1) * b] = D[i]
        if i + 1 < N:
            A[(i + 1) * b:(i + 2) * b, i * b:(i + 1) * b] = O[i]
            A[i * b:(i + 1) * b, (i + 1) * b:(i + 2) * b] = O[i].T
    if B is None:
        return A
    Bf = B.reshape(N * b, -1)
    return np.block([[A, Bf], [Bf.T, HLL]])


def jacobi_scale(H):
    return np.sqrt(np.diag(H))


def scaled_cond(H):
    """condition number of the Jacobi-scaled H (tests/test_gpu_marginals.py:tol_of)"""
    s = jacobi_scale(H)
    return float(np.linalg.cond(H / np.outer(s, s)))


def step_tol(H):
    """tests/test_gpu_marginals.py's rule: max(1e-10, 100 eps kappa_s), which must stay <= 1e-7"""
    kappa = scaled_cond(H)
    tol = max(1e-10, 100 * EPS * kappa)
    assert tol <= 1e-7, kappa
    return tol


class FactorLists:
    """Records the set_* / add_* calls of a solver-like object (arguments copied as arrays)."""

    def __init__(self, d, landmark_dim=0):
        self.d, self.b, self.ld = d, 2 * d, landmark_dim
        self.calls = []
        self.N = self.L = 0

    def __getattr__(self, name):
        if not (name.startswith("set_") or name.startswith("add_")):
            raise AttributeError(name)

        def record(*args):
            args = tuple(None if a is None else np.array(a, copy=True) for a in args)
            if name == "set_states":
                self.N = len(args[0])
            if name == "set_landmarks":
                self.L = len(np.asarray(args[0]).reshape(-1, self.ld))
            self.calls.append((name, args))
            return 0
        return record

    def compile(self):
        return 0

    def args_of(self, name):
        return [a for n, a in self.calls if n == name]

    def first_args(self, *names):
        got = [np.asarray(a[0], dtype=int).ravel() for n, a in self.calls if n in names]
        return np.concatenate(got) if got else np.zeros(0, dtype=int)

    def replay(self, solver, edit=None):
        """edit(name, args) -> args: a chance to change a call on its way (e.g. translate its positions)"""
        for name, args in self.calls:
            if edit is not None:
                args = edit(name, tuple(None if a is None else a.copy() for a in args))
            getattr(solver, name)(*args)
        solver.compile()
        return solver

    def meas(self):
        out = {}
        for name, k in MEAS_CALL.items():
            idx = self.first_args(name)
            if len(idx):
                out[k] = idx
        return out

    def row_map(self):
        return row_map(self.N, self.d, self.first_args("add_gp_priors", "add_gp_priors_qc"), self.first_args("add_vel_priors"),
                       self.first_args("add_pose_priors"), self.first_args("add_between"), self.meas())

    def n_rows(self):
        """the row count the factor lists imply"""
        n = self.b * len(self.first_args("add_gp_priors", "add_gp_priors_qc"))
        n += self.d * (len(self.first_args("add_vel_priors")) + len(self.first_args("add_pose_priors")) + len(self.first_args("add_between")))
        return n + sum(MEAS_ROWS[k] * len(idx) for k, idx in self.meas().items())

    def lprior(self):
        a = self.args_of("add_landmark_priors")
        if not a:
            return None
        return (np.concatenate([np.asarray(x[0], dtype=int).ravel() for x in a]),
                np.concatenate([np.asarray(x[2], dtype=float).reshape(-1, self.ld) for x in a]),
                np.concatenate([np.asarray(x[1], dtype=float).reshape(-1, self.ld) for x in a]))

    def assemble(self, rows, landmarks=None):
        """normal equations of a handle's get_rows() output for this graph; landmarks: their current values (for gL)"""
        LR, E, Mm, Lm = rows
        lp = self.lprior()
        if lp is not None:
            idx, sig, prior = lp
            lp = (idx, sig) if landmarks is None else (idx, sig, np.asarray(landmarks).reshape(-1, self.ld)[idx] - prior)
        return assemble(self.N, self.b, self.row_map().left, LR, E, Mm, Lm, self.L, self.ld, lp)
