"""Numpy model of gpslam_hip_get_state_pair_marginals (gpslam_amd/csrc/marginals_pairs.hip): Sigma_{a,b} of any two states from
what gpslam_hip_marginals leaves on the device.

The chain part A (block tridiagonal, N blocks of b x b) is factored as k_mg_forward does: chunks of CHUNK items, the first item of
a chunk its separator, the interiors eliminated in order; per interior j the record [P_j^-1 | U_j | V_j] (U_j = P_j^-1 A'_{j,j+1},
V_j = P_j^-1 A'_{j,s}); the separators form a system of the same kind one level up, until one block is left (Sigma_top).  In
x_j = P_j^-1 r_j - U_j x_{j+1} - V_j x_s the records are a block L D L^T of A in the elimination order, so

    A^-1_{a,b} = (L^-1 E_a)^T D^-1 (L^-1 E_b) = sum over eliminated items i of (r^a_i)^T P_i^-1 r^b_i + (r^a_top)^T Sigma_top r^b_top,

r^a, r^b the forward sweeps of the identity block at a and at b:  r_{j+1} -= U_j^T r_j,  r_s -= V_j^T r_j  (the last interior's
U_j^T r_j goes to the right separator).  At every level a sweep is non-zero on at most two adjacent items (p, p + 1) and touches
only the interiors from there to the end of p's chunk; the two sweeps meet only where both are in the same chunk.  No backward
walk and nothing stored per level: 6 block products per common interior, 2 per interior that only one side visits.
"""
import numpy as np

CHUNK = 16


def random_chain(N, b, rng, coupling=0.9):
    """SPD block-tridiagonal A = J^T J-like: D (N, b, b) and O (N, b, b) with O_i = A_{i+1,i} (the last one unused, zero)."""
    G = rng.standard_normal((N + 1, 2 * b, 2 * b)) * coupling
    D = np.zeros((N, b, b))
    O = np.zeros((N, b, b))
    for i in range(N):
        D[i] += np.eye(b) * 0.05
    for i in range(N - 1):        # a factor between i and i + 1: rows G[i] = [Gl | Gr]
        Gl, Gr = G[i][:, :b], G[i][:, b:]
        D[i] += Gl.T @ Gl
        D[i + 1] += Gr.T @ Gr
        O[i] = Gr.T @ Gl
    D[0] += G[N][:b, :b].T @ G[N][:b, :b] + np.eye(b)     # the anchor
    return D, O


def dense(D, O):
    N, b = D.shape[0], D.shape[1]
    A = np.zeros((N * b, N * b))
    for i in range(N):
        A[i * b:(i + 1) * b, i * b:(i + 1) * b] = D[i]
        if i + 1 < N:
            A[(i + 1) * b:(i + 2) * b, i * b:(i + 1) * b] = O[i]
            A[i * b:(i + 1) * b, (i + 1) * b:(i + 2) * b] = O[i].T
    return A


def factor(D, O):
    """The hierarchy as k_mg_forward / k_mg_top leave it: ([(n_l, fac_l)] for the levels below the top, Sigma_top).
    fac_l: (n_l, 3, b, b) = [P^-1 | U | V] of every interior item (separators' records stay zero)."""
    b = D.shape[1]
    levels = []
    D, O = D.copy(), O.copy()
    while D.shape[0] > 1:
        n = D.shape[0]
        nu = (n + CHUNK - 1) // CHUNK
        fac = np.zeros((n, 3, b, b))
        upD, upO, upAdd = np.zeros((nu, b, b)), np.zeros((nu, b, b)), np.zeros((nu, b, b))
        for k in range(nu):
            s, e = k * CHUNK, min(k * CHUNK + CHUNK, n)
            right = e < n
            Ds = D[s].copy()
            if e == s + 1:
                upD[k] = Ds
                upO[k] = O[s] if right else 0.0
                continue
            P, F = D[s + 1].copy(), O[s].copy()
            for j in range(s + 1, e):
                Pi = np.linalg.inv(P)
                E = O[j].T if j + 1 < n else np.zeros((b, b))
                U, V = Pi @ E, Pi @ F
                fac[j] = Pi, U, V
                Ds -= F.T @ V
                if j + 1 < e:
                    P = D[j + 1] - E.T @ U
                    F = -E.T @ V
                else:
                    if right:
                        upAdd[k + 1] = E.T @ U
                    upO[k] = -E.T @ V
            upD[k] = Ds
        levels.append((n, fac))
        D, O = upD - upAdd, upO
    return levels, np.linalg.inv(D[0])


class _Side:
    """One forward sweep: the right-hand side on items p (R0) and p + 1 (R1, if has1) of the current level."""

    def __init__(self, p, b):
        self.p, self.R0, self.R1, self.has1 = p, np.eye(b), np.zeros((b, b)), False

    def rhs(self, j):
        if j == self.p:
            return self.R0
        if self.has1 and j == self.p + 1:
            return self.R1
        return None


def chain_pair(levels, top, a, b, count=None):
    """A^-1_{a,b} (rows: state a) by the two forward sweeps; count: a one-element list that takes the number of block products."""
    bs = top.shape[0]
    sides = [_Side(a, bs), _Side(b, bs)]
    acc = np.zeros((bs, bs))
    nprod = 0
    for n, fac in levels:
        c = [sd.p // CHUNK for sd in sides]
        e = [min(ci * CHUNK + CHUNK, n) for ci in c]
        start = [max(sd.p, ci * CHUNK + 1) for sd, ci in zip(sides, c)]
        cur = [None, None]                       # r_j of each side at the item the loop stands on (None: zero so far)
        sep = [np.zeros((bs, bs)), np.zeros((bs, bs))]
        carry = [None, None]                     # what the last interior hands to the right separator
        groups = [[0, 1]] if c[0] == c[1] else [[0], [1]]
        for g in groups:
            for j in range(min(start[t] for t in g), e[g[0]]):
                Pi, U, V = fac[j]
                for t in g:
                    if j < start[t]:
                        continue
                    add = sides[t].rhs(j)
                    if add is not None:
                        cur[t] = add if cur[t] is None else cur[t] + add
                if len(g) == 2 and cur[0] is not None and cur[1] is not None:
                    acc += cur[0].T @ (Pi @ cur[1])
                    nprod += 2
                for t in g:
                    if cur[t] is None:
                        continue
                    sep[t] -= V.T @ cur[t]
                    nxt = -(U.T @ cur[t])
                    nprod += 2
                    if j + 1 < e[t]:
                        cur[t] = nxt
                    else:
                        carry[t] = nxt
                        cur[t] = None
        for t, sd in enumerate(sides):
            s = c[t] * CHUNK
            R0 = sep[t] + (sd.R0 if sd.p == s else 0.0)
            has1 = e[t] < n
            R1 = np.zeros((bs, bs))
            if has1:
                if carry[t] is not None:
                    R1 = R1 + carry[t]
                right = sd.rhs(e[t])            # the right separator itself carried a right-hand side
                if right is not None:
                    R1 = R1 + right
            sd.p, sd.R0, sd.R1, sd.has1 = c[t], R0, R1, has1
    acc += sides[0].R0.T @ (top @ sides[1].R0)
    nprod += 2
    if count is not None:
        count[0] = nprod
    return acc


def lowrank_single(Y, K, a, b):
    """+ Y_a K Y_b^T on a single-pass handle.  Y: (N, m, bs) as the level-0 solution stores it (column q of state i: Y[i, q, :])."""
    return Y[a].T @ K @ Y[b]


def lowrank_passes(W, Sinv, Z, Minv, a, b, bs):
    """+ W_a S^-1 W_b^T - Z_a M^-1 Z_b^T on a column-pass handle.  W: (N, nl, bs); Z: (rows, ldz), row i bs + r; Minv (ldz, ldz)."""
    Za, Zb = Z[a * bs:(a + 1) * bs], Z[b * bs:(b + 1) * bs]
    out = -Za @ Minv @ Zb.T
    if W.shape[1]:
        out = out + W[a].T @ Sinv @ W[b]
    return out


def border_problem(N, bs, nl, ncr, rng):
    """A chain with nl landmark columns and ncr closure rows, in both storage forms.  Returns D, O, H (dense, states then landmarks),
    and the terms Y, K (single pass), W, Sinv, Z (padded), Minv (padded)."""
    D, O = random_chain(N, bs, rng)
    A = dense(D, O)
    n = N * bs
    Bm = np.zeros((n, nl))
    for c in range(nl):           # a landmark column touches a few states
        for i in rng.choice(N, size=min(N, 3), replace=False):
            Bm[i * bs:(i + 1) * bs, c] = rng.standard_normal(bs) * 0.5
    g = rng.standard_normal((nl, nl))
    HLL = np.eye(nl) * 4.0 + g.T @ g
    Uc = np.zeros((ncr, n))
    for r in range(ncr):
        i, j = rng.choice(N, size=2, replace=False) if N > 1 else (0, 0)
        Uc[r, i * bs:(i + 1) * bs] = rng.standard_normal(bs) * 0.7
        Uc[r, j * bs:(j + 1) * bs] += rng.standard_normal(bs) * 0.7
    H = np.zeros((n + nl, n + nl))
    H[:n, :n] = A + Uc.T @ Uc
    H[:n, n:] = Bm
    H[n:, :n] = Bm.T
    H[n:, n:] = HLL + Bm.T @ np.linalg.solve(H[:n, :n], Bm)      # keeps H positive definite whatever B is
    Ainv = np.linalg.inv(A)
    Zf = Ainv @ Uc.T
    M = np.eye(ncr) + 0.5 * (Uc @ Zf + (Uc @ Zf).T)
    Mi = np.linalg.inv(M)
    Wf = np.linalg.solve(H[:n, :n], Bm)
    Si = np.linalg.inv(H[n:, n:] - Bm.T @ Wf) if nl else np.zeros((0, 0))
    m = nl + ncr
    Y = np.zeros((N, m, bs))
    for i in range(N):
        Y[i, :nl] = Wf[i * bs:(i + 1) * bs].T
        Y[i, nl:] = Zf[i * bs:(i + 1) * bs].T
    K = np.zeros((m, m))
    K[:nl, :nl] = Si
    K[nl:, nl:] = -Mi
    ldz = (ncr + 15) // 16 * 16
    Zp = np.zeros((n + 16, ldz))
    Zp[:n, :ncr] = Zf
    Mp = np.zeros((ldz, ldz))
    Mp[:ncr, :ncr] = Mi
    return D, O, H, Y, K, Y[:, :nl].copy(), Si, Zp, Mp


def corr_err(got, want, sa, sb):
    """max |got - want|_rc / (sigma_r sigma_c): the error in correlation units"""
    return float(np.max(np.abs(got - want) / np.outer(sa, sb)))
