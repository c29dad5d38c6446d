"""CPU: the numpy model of gpslam_hip_marginals against dense inverses (tests/marginals_model.py)."""
import numpy as np
import pytest

import marginals_model as MM

C = MM.CHUNK


def corr_err(Shat, S, diag):
    """|Shat - S| / sqrt(S_kk S_ll): the error in correlation units"""
    return np.max(np.abs(Shat - S) / np.sqrt(np.outer(diag, diag)))


@pytest.mark.parametrize("b,N", [(b, N) for b in (4, 6, 12) for N in (1, 2, C - 1, C, C + 1, C * C + 5)] + [(6, C * C * C + 3)])
def test_selected_inversion_matches_dense_inverse(b, N):
    D, O = MM.random_chain(N, b, seed=N + b)
    Sd, Sn = MM.selinv(D, O)
    if N * b <= 3000:
        Sig = np.linalg.inv(MM.dense(D, O))
        diag = np.diag(Sig)
        for i in range(N):
            blk = Sig[i * b:(i + 1) * b, i * b:(i + 1) * b]
            assert corr_err(Sd[i], blk, diag[i * b:(i + 1) * b]) < 1e-12
            if i + 1 < N:
                nxt = Sig[i * b:(i + 1) * b, (i + 1) * b:(i + 2) * b]
                assert np.max(np.abs(Sn[i] - nxt)) / np.sqrt(diag[i * b:(i + 1) * b].max() * diag[(i + 1) * b:(i + 2) * b].max()) < 1e-12
        assert np.all(Sn[-1] == 0.0)
    else:   # three levels: check through A Sigma = I on the computed blocks
        for i in range(N):
            r = D[i] @ Sd[i]
            if i + 1 < N:
                r += O[i].T @ Sn[i].T
            if i > 0:
                r += O[i - 1] @ Sn[i - 1]
            assert np.max(np.abs(r - np.eye(b))) < 1e-11


@pytest.mark.parametrize("b,nl,nclo", [(6, 0, 2), (6, 8, 0), (6, 4, 3), (12, 9, 2), (4, 27, 0), (4, 2, 12)])
def test_lowrank_term_matches_dense_inverse(b, nl, nclo):
    """landmarks (B, H_LL) and closures (J_c) folded into the chain's inverse: the blocks of the dense inverse of the whole H"""
    rng = np.random.default_rng(100 * b + nl + nclo)
    N = 40
    D, O = MM.random_chain(N, b, seed=7)
    A = MM.dense(D, O)
    d = b // 2
    Jc = None
    if nclo:
        Jc = np.zeros((nclo * d, N * b))
        for k in range(nclo):
            i, j = sorted(rng.choice(N, 2, replace=False))
            Jc[k * d:(k + 1) * d, i * b:i * b + d] = rng.standard_normal((d, d))
            Jc[k * d:(k + 1) * d, j * b:j * b + d] = rng.standard_normal((d, d))
    B = 0.2 * rng.standard_normal((N * b, nl)) if nl else None
    HLL = None
    if nl:
        G = rng.standard_normal((nl, nl))
        HLL = G @ G.T + (nl + 4.0) * np.eye(nl) + B.T @ np.linalg.solve(A, B)
    H = A + (Jc.T @ Jc if Jc is not None else 0.0)
    if nl:
        H = np.block([[H, B], [B.T, HLL]])
    Sig = np.linalg.inv(H)
    kappa = np.linalg.cond(H / np.sqrt(np.outer(np.diag(H), np.diag(H))))
    Sxx, SxL, SLL = MM.lowrank(np.linalg.inv(A), B, Jc, HLL)
    n = N * b
    diag = np.diag(Sig)
    tol = max(1e-10, 100 * np.finfo(float).eps * kappa)
    assert corr_err(Sxx, Sig[:n, :n], diag[:n]) < tol
    if nl:
        assert corr_err(SLL, Sig[n:, n:], diag[n:]) < tol
        assert np.max(np.abs(SxL - Sig[:n, n:]) / np.sqrt(np.outer(diag[:n], diag[n:]))) < tol


@pytest.mark.parametrize("dt,tau", [(0.1, 0.03), (1.0, 0.5), (2.5, 0.1), (0.01, 0.0099)])
def test_gp_conditional_pose_block_closed_form(dt, tau):
    Qc = np.array([[2.0, 0.3, 0.1], [0.3, 1.0, 0.2], [0.1, 0.2, 0.5]])
    Qt = MM.gp_conditional(dt, tau, Qc)
    ref = MM.gp_c(dt, tau) * Qc
    assert np.max(np.abs(Qt[:3, :3] - ref)) <= 1e-9 * np.max(np.abs(Qc)) * max(dt ** 3, 1e-12) + 1e-15
