"""Dense-numpy model of the marginals on the segmented landmark path: nested dissection along the chain with fat
separators, and the selected inversion back through it.  Everything is written block by block the way the device kernels walk it;
the dense H only supplies the blocks.

    states 0 .. N-1 (b coordinates each); cut k is state cuts[k]; fat block k = [cut state k | its landmark coordinates] (NB wide);
    segment s = the states strictly between cut s and cut s + 1; its border B_s = [fat block s | fat block s + 1].

Forward half (what a solve at lambda = 0 leaves behind):
    per segment  A_s = L L^T along the chain (W_j = L_jj^-1, E_j = W_j H[j, j+1]),  Y = L^-1 H[I_s, B_s];
    fat chain    D_k = H[F_k, F_k] - (Y^T Y parts of the two neighbouring segments),  link_k = H[F_k+1, F_k] - (Y^T Y)[right, left];
    cyclic reduction over level sets (levels()): block m between l and r:  D_m = L_m L_m^T, P = L_m^-1 H[m, l], Q = L_m^-1 H[m, r],
                 D_l -= P^T P, D_r -= Q^T Q, new H[r, l] = -Q^T P.
Selected inversion (steps 1-4 of the issue):
    1. top block Sigma = D^-1; per level in reverse, with U = P S_ll + Q S_rl, V = P S_lr + Q S_rr:
           S_ml = -L_m^-T U,  S_mr = -L_m^-T V,  S_mm = L_m^-T (I + U P^T + V Q^T) L_m^-1;
       adjacent pairs are keyed by the LINK index of the pair (pair[lk] = Sigma_{left, right}): the pair (l, r) of the level above
       is the new link the elimination of m created, the pairs (l, m) and (m, r) are the links it consumed.
    2. G_j = W_j^T (Y_j - E_j G_{j+1}) backwards along the segment (G = A_s^-1 H[I_s, B_s]: Y carries H's own sign);
    3. Z_jj = W_j^T W_j + M_j Z_{j+1,j+1} M_j^T,  Z_{j,j+1} = -M_j Z_{j+1,j+1},  M_j = W_j^T E_j;
    4. T_i = G_i Sigma_BB:  Sigma_ii = Z_ii + T_i G_i^T,  Sigma_{i,i+1} = Z_{i,i+1} + T_i G_{i+1}^T,  Sigma_{i,F} = -T_i."""
import numpy as np


def levels(K):
    """FatSepPlan::build_levels without keep_last: per level a list of (m, l, r, link(l -> m), link(m -> r), new link(l -> r));
    r and the two links behind it are -1 at the chain's end.  Returns (levels, top, nlinks)."""
    active = list(range(K))
    linkidx = list(range(K - 1))
    next_link = K - 1
    out = []
    while len(active) > 1:
        n = len(active)
        lev, nlink = [], []
        for q in range(1, n, 2):
            r = active[q + 1] if q + 1 < n else -1
            lk_new = -1
            if r >= 0:
                lk_new = next_link
                next_link += 1
                nlink.append(lk_new)
            lev.append((active[q], active[q - 1], r, linkidx[q - 1], linkidx[q] if r >= 0 else -1, lk_new))
        out.append(lev)
        active = active[0::2]
        linkidx = nlink
    return out, active[0], max(next_link, 1)


def random_system(rng, b, cuts, NB, rows_per_lm=3):
    """A random SPD H = J^T J + I of the segmented shape.  Returns (H, state index lists, fat index lists)."""
    N, K = cuts[-1] + 1, len(cuts)
    nlc = NB - b
    n = N * b + K * nlc
    sidx = [np.arange(s * b, (s + 1) * b) for s in range(N)]
    lidx = [N * b + k * nlc + np.arange(nlc) for k in range(K)]
    fidx = [np.concatenate([sidx[cuts[k]], lidx[k]]) for k in range(K)]
    rows = []
    for s in range(N - 1):                      # chain factors
        J = np.zeros((b, n))
        J[:, sidx[s]] = rng.normal(size=(b, b))
        J[:, sidx[s + 1]] = rng.normal(size=(b, b))
        rows.append(J)
    for k in range(K):                          # landmark rows: states of the two segments next to cut k (cut states included)
        lo, hi = cuts[max(k - 1, 0)], cuts[min(k + 1, K - 1)] - 1
        for c in range(nlc):
            for _ in range(rows_per_lm):
                s = int(rng.integers(lo, hi + 1))
                J = np.zeros((1, n))
                J[0, sidx[s]] = rng.normal(size=b)
                J[0, sidx[s + 1]] = rng.normal(size=b)
                J[0, lidx[k][c]] = rng.normal()
                if c + 1 < nlc:
                    J[0, lidx[k][c + 1]] = rng.normal()
                rows.append(J)
    J = np.vstack(rows)
    return J.T @ J + np.eye(n), sidx, fidx


def segmented_marginals(H, b, cuts, sidx, fidx):
    """Steps 1-4.  Returns dict: Sd[i], Sn[i] (state blocks), fat[k], fatpair[k] (Sigma_{k,k+1}), sxF[i] = Sigma_{i, B_s} (interior
    states only, columns in border order [fat s | fat s + 1])."""
    K, N, NB = len(cuts), cuts[-1] + 1, len(fidx[0])
    blk = lambda I, J: H[np.ix_(I, J)]
    # ---- forward half
    seg = []
    D = [blk(fidx[k], fidx[k]).copy() for k in range(K)]
    lv, top, nlinks = levels(K)
    link = [None] * nlinks
    for k in range(K - 1):
        link[k] = blk(fidx[k + 1], fidx[k]).copy()
    for s in range(K - 1):
        ints = list(range(cuts[s] + 1, cuts[s + 1]))
        if not ints:
            seg.append(None)
            continue
        I = np.concatenate([sidx[j] for j in ints])
        Bs = np.concatenate([fidx[s], fidx[s + 1]])
        L = np.linalg.cholesky(blk(I, I))
        n = len(ints)
        W = [np.linalg.inv(L[j * b:(j + 1) * b, j * b:(j + 1) * b]) for j in range(n)]
        E = [W[j] @ blk(sidx[ints[j]], sidx[ints[j] + 1]) for j in range(n)]     # (the last one couples to the cut: unused)
        Y = np.linalg.solve(L, blk(I, Bs))
        A = Y.T @ Y
        D[s] -= A[:NB, :NB]
        D[s + 1] -= A[NB:, NB:]
        link[s] -= A[NB:, :NB]
        seg.append((ints, W, E, Y))
    Lm, P, Q = {}, {}, {}
    for lev in lv:
        for (m, l, r, lk_lm, lk_mr, lk_new) in lev:
            Lm[m] = np.linalg.cholesky(D[m])
            P[m] = np.linalg.solve(Lm[m], link[lk_lm])
            D[l] = D[l] - P[m].T @ P[m]
            if r >= 0:
                Q[m] = np.linalg.solve(Lm[m], link[lk_mr].T)
                D[r] = D[r] - Q[m].T @ Q[m]
                link[lk_new] = -Q[m].T @ P[m]
    # ---- 1. the fat chain's selected inverse
    Sf = [None] * K
    pair = [None] * nlinks
    Sf[top] = np.linalg.inv(D[top])
    for lev in reversed(lv):
        for (m, l, r, lk_lm, lk_mr, lk_new) in lev:
            Wm = np.linalg.inv(Lm[m])
            U = P[m] @ Sf[l]
            V = None
            if r >= 0:
                U = U + Q[m] @ pair[lk_new].T
                V = P[m] @ pair[lk_new] + Q[m] @ Sf[r]
            Sml = -Wm.T @ U
            T = Wm.T - Sml @ P[m].T
            pair[lk_lm] = Sml.T
            if r >= 0:
                Smr = -Wm.T @ V
                T = T - Smr @ Q[m].T
                pair[lk_mr] = Smr
            Sf[m] = T @ Wm
    out = {"Sd": [None] * N, "Sn": [np.zeros((b, b)) for _ in range(N)], "fat": Sf, "fatpair": pair[:K - 1], "sxF": {}}
    for k in range(K):
        out["Sd"][cuts[k]] = Sf[k][:b, :b]
    # ---- 2-4. the segments
    for s in range(K - 1):
        SBB = np.block([[Sf[s], pair[s]], [pair[s].T, Sf[s + 1]]])
        if seg[s] is None:
            out["Sn"][cuts[s]] = pair[s][:b, :b]
            continue
        ints, W, E, Y = seg[s]
        n = len(ints)
        G, Zd, Zn = [None] * n, [None] * n, [None] * n
        for j in range(n - 1, -1, -1):
            Yj = Y[j * b:(j + 1) * b]
            if j == n - 1:
                G[j] = W[j].T @ Yj
                Zd[j] = W[j].T @ W[j]
            else:
                Mj = W[j].T @ E[j]
                G[j] = W[j].T @ (Yj - E[j] @ G[j + 1])
                Zn[j] = -Mj @ Zd[j + 1]
                Zd[j] = W[j].T @ W[j] - Zn[j] @ Mj.T
        for j in range(n):
            i = ints[j]
            T = G[j] @ SBB
            out["Sd"][i] = Zd[j] + T @ G[j].T
            out["sxF"][i] = -T
            if j + 1 < n:
                out["Sn"][i] = Zn[j] + T @ G[j + 1].T
            else:
                out["Sn"][i] = -T[:, NB:NB + b]                 # Sigma_{last interior, right cut}
            if j == 0:
                out["Sn"][cuts[s]] = -T[:, :b].T                # Sigma_{left cut, first interior}
    return out
